"""GPU tests for the fused MLP kernels (stoix_amd/ops/csrc/mlp.hip) against
plain-PyTorch fp32 references."""
import math

import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

requires_gpu = pytest.mark.skipif(not torch.cuda.is_available(), reason="no GPU")


@pytest.fixture(scope="module")
def ext():
    from stoix_amd import ops

    e = ops.ext(required=True)
    assert e is not None
    return e


@requires_gpu
def test_mfma_probe_layout(ext):
    """The fused kernels assume variant-0 operand layout for
    v_mfma_f32_16x16x32_bf16 (lane l: A[m=l&15][k=(l>>4)*8+j]). The probe
    computes D = A@B under both candidate layouts; variant 0 must match."""
    g = torch.Generator().manual_seed(0)
    A = torch.randn(16, 32, generator=g).bfloat16().cuda()
    # asymmetric B (guide: symmetric B passes transposed C-writes)
    B = (torch.randn(32, 16, generator=g) * torch.linspace(0.5, 2.0, 16)).bfloat16().cuda()
    D0 = torch.zeros(16, 16, device="cuda")
    D1 = torch.zeros(16, 16, device="cuda")
    ext.mfma_probe(A, B, D0, D1)
    ref = (A.float() @ B.float()).cpu()
    err0 = (D0.cpu() - ref).abs().max().item()
    err1 = (D1.cpu() - ref).abs().max().item()
    assert err0 < 0.1, f"variant-0 MFMA layout wrong (err0={err0}, err1={err1})"


@requires_gpu
def test_silu_kernels(ext):
    g = torch.Generator().manual_seed(1)
    z = torch.randn(1000, 256, generator=g).bfloat16().cuda()
    dh = torch.randn(1000, 256, generator=g).bfloat16().cuda()
    h = torch.empty_like(z)
    dz = torch.empty_like(z)
    ext.silu_fwd(z, h)
    ext.silu_bwd(dh, z, dz)
    zf = z.float()
    torch.testing.assert_close(h.float(), F.silu(zf), rtol=1e-2, atol=1e-2)
    s = torch.sigmoid(zf)
    ref = dh.float() * (s * (1 + zf * (1 - s)))
    torch.testing.assert_close(dz.float(), ref, rtol=2e-2, atol=2e-2)


def _mk_weights(H, OBS, ACT, device):
    """W1 is zero-padded to the MFMA K-step (32 cols) like the fused engine
    stores it (mlp.hip reads W1 with row stride K1P)."""
    K1P = (OBS + 31) & ~31
    g = torch.Generator().manual_seed(7)
    r = lambda *s: torch.randn(*s, generator=g).to(device) * (1.0 / math.sqrt(s[-1]))

    def rpad(H_, OBS_):
        w = torch.zeros(H_, K1P, device=device)
        w[:, :OBS_] = r(H_, OBS_)
        return w

    W1a, b1a = rpad(H, OBS), torch.randn(H, generator=g).to(device) * 0.1
    W2a, b2a = r(H, H), torch.randn(H, generator=g).to(device) * 0.1
    Wha = torch.zeros(16, H, device=device)
    Wha[0:ACT] = r(ACT, H)
    Wha[8 : 8 + ACT] = r(ACT, H)
    bha = torch.zeros(16, device=device)
    bha[0:ACT] = torch.randn(ACT, generator=g).to(device) * 0.1
    bha[8 : 8 + ACT] = torch.randn(ACT, generator=g).to(device) * 0.1
    W1c, b1c = rpad(H, OBS), torch.randn(H, generator=g).to(device) * 0.1
    W2c, b2c = r(H, H), torch.randn(H, generator=g).to(device) * 0.1
    Wvc = r(H)
    bvc = torch.randn(1, generator=g).to(device) * 0.1
    return W1a, b1a, W2a, b2a, Wha, bha, W1c, b1c, W2c, b2c, Wvc, bvc


def _eager_forward(obs, W1, b1, W2, b2):
    h = F.silu(F.linear(obs, W1[:, : obs.shape[1]], b1))
    return F.silu(F.linear(h, W2, b2))


@requires_gpu
@pytest.mark.parametrize("H,OBS,ACT", [(256, 27, 8), (256, 64, 4), (128, 27, 8), (512, 27, 8)])
def test_policy_value_step_matches_eager(ext, H, OBS, ACT):
    device = "cuda"
    B = 256
    (W1a, b1a, W2a, b2a, Wha, bha, W1c, b1c, W2c, b2c, Wvc, bvc) = _mk_weights(
        H, OBS, ACT, device
    )
    obs = torch.randn(B, OBS, device=device)
    e = torch.zeros(0, device=device)
    action = torch.zeros(B, ACT, device=device)
    logp = torch.zeros(B, device=device)
    value = torch.zeros(B, device=device)
    obs_mirror = torch.zeros(B, OBS, device=device)
    draw = torch.zeros(1, dtype=torch.int32, device=device)
    bf = lambda t: t.bfloat16()
    ext.policy_value_step(
        obs, bf(W1a), b1a, bf(W2a), b2a, bf(Wha), bha, bf(W1c), b1c, bf(W2c),
        b2c, bf(Wvc), bvc, obs_mirror, action, logp, value, e, e,
        1e-3, 1.0, 0.0, 0.0, 1, 1234, draw, 0, 1,
    )
    torch.cuda.synchronize()
    assert draw.item() == 1  # counter bumped
    torch.testing.assert_close(obs_mirror, obs)
    # greedy=1: action = tanh(loc); logp computed at eps=0 (u = loc)
    h2a = _eager_forward(obs, W1a, b1a, W2a, b2a)
    loc = F.linear(h2a, Wha[0:ACT], bha[0:ACT])
    spre = F.linear(h2a, Wha[8 : 8 + ACT], bha[8 : 8 + ACT])
    sigma = F.softplus(spre) + 1e-3
    torch.testing.assert_close(action, torch.tanh(loc), rtol=3e-2, atol=3e-2)
    log_det = 2.0 * (math.log(2.0) - loc - F.softplus(-2.0 * loc))
    logp_ref = (-sigma.log() - 0.5 * math.log(2 * math.pi) - log_det).sum(-1)
    torch.testing.assert_close(logp, logp_ref, rtol=5e-2, atol=0.2)
    h2c = _eager_forward(obs, W1c, b1c, W2c, b2c)
    v_ref = F.linear(h2c, Wvc.view(1, -1), bvc).view(-1)
    torch.testing.assert_close(value, v_ref, rtol=3e-2, atol=5e-2)

    # value_forward agrees with the critic part
    v2 = torch.zeros(B, device=device)
    ext.value_forward(obs, bf(W1c), b1c, bf(W2c), b2c, bf(Wvc), bvc, v2, e, e)
    torch.testing.assert_close(v2, value, rtol=1e-3, atol=1e-3)


@requires_gpu
def test_policy_step_sampling_statistics(ext):
    """Non-greedy sampling: actions ~ tanh(N(loc, sigma)); mean/std of atanh
    over many draws must approach loc/sigma, and draws differ per step."""
    device = "cuda"
    H, OBS, ACT, B = 256, 27, 8, 4096
    w = _mk_weights(H, OBS, ACT, device)
    (W1a, b1a, W2a, b2a, Wha, bha, W1c, b1c, W2c, b2c, Wvc, bvc) = w
    obs = torch.randn(B, OBS, device=device) * 0.0  # identical rows
    e = torch.zeros(0, device=device)
    action = torch.zeros(B, ACT, device=device)
    logp = torch.zeros(B, device=device)
    value = torch.zeros(B, device=device)
    draw = torch.zeros(1, dtype=torch.int32, device=device)
    bf = lambda t: t.bfloat16()
    samples = []
    for _ in range(4):
        ext.policy_value_step(
            obs, bf(W1a), b1a, bf(W2a), b2a, bf(Wha), bha, bf(W1c), b1c,
            bf(W2c), b2c, bf(Wvc), bvc, e, action, logp, value, e, e,
            1e-3, 1.0, 0.0, 0.0, 0, 99, draw, 0, 1,
        )
        samples.append(action.clone())
    torch.cuda.synchronize()
    assert draw.item() == 4
    assert not torch.allclose(samples[0], samples[1])  # fresh draws per step
    u = torch.atanh(torch.cat(samples).clamp(-0.999999, 0.999999))
    h2a = _eager_forward(obs[:1], W1a, b1a, W2a, b2a)
    loc = F.linear(h2a, Wha[0:ACT], bha[0:ACT])[0]
    sigma = (F.softplus(F.linear(h2a, Wha[8:16], bha[8:16])) + 1e-3)[0]
    torch.testing.assert_close(u.mean(0), loc, rtol=0.1, atol=0.05 * sigma.max().item() + 0.02)
    torch.testing.assert_close(u.std(0), sigma, rtol=0.1, atol=0.05)


@requires_gpu
def test_ppo_head_loss_kernel_matches_reference(ext):
    """Kernel fwd losses + analytic bwd vs the fp32 torch reference
    (tests/test_fused_math.py validated that reference against autograd).
    The head projections are GEMMs outside the kernel now; the kernel gets
    heads [B,16] (loc|spre) and v [B] directly."""
    from tests.test_fused_math import closed_form_grads

    device = "cuda"
    ACT, B = 8, 512
    g = torch.Generator().manual_seed(3)
    loc = torch.randn(B, ACT, generator=g).to(device) * 0.5
    spre = torch.randn(B, ACT, generator=g).to(device)
    v_pred = torch.randn(B, generator=g).to(device)
    heads = torch.cat([loc, spre], dim=1).bfloat16()
    v16 = v_pred.bfloat16()
    action = (torch.rand(B, ACT, generator=g).to(device) * 1.8 - 0.9)
    old_logp = torch.randn(B, generator=g).to(device)
    old_value = torch.randn(B, generator=g).to(device)
    adv = torch.randn(B, generator=g).to(device)
    targets = torch.randn(B, generator=g).to(device)
    dhead = torch.zeros(B, 16, device=device, dtype=torch.bfloat16)
    dv = torch.zeros(B, 1, device=device, dtype=torch.bfloat16)
    metrics = torch.zeros(3, device=device)
    draw = torch.zeros(1, dtype=torch.int32, device=device)
    clip_eps, vf_coef = 0.2, 0.5
    # ent_coef=0 so the (stochastic) entropy term has no gradient; the
    # entropy VALUE is still checked for plausibility below
    dv16 = torch.zeros(B, 16, device=device, dtype=torch.bfloat16)
    ext.ppo_head_loss(
        heads, v16, action, old_logp, old_value, adv, targets, dhead, dv,
        dv16, metrics, clip_eps, 0.0, vf_coef, 1e-3, 1.0, 0.0, 0.0, 42, draw,
        0, 1,
    )
    torch.cuda.synchronize()
    assert draw.item() == 1

    locf = heads.float()[:, 0:ACT]
    spref = heads.float()[:, 8 : 8 + ACT]
    sigma = F.softplus(spref) + 1e-3
    vf = v16.float()
    y = action.clamp(-1 + 1e-3, 1 - 1e-3)
    u = torch.atanh(y)
    z = (u - locf) / sigma
    log_det = 2.0 * (math.log(2.0) - u - F.softplus(-2.0 * u))
    logp_new = (-0.5 * z * z - sigma.log() - 0.5 * math.log(2 * math.pi) - log_det).sum(-1)
    ratio = torch.exp(logp_new - old_logp)
    l1, l2 = ratio * adv, ratio.clamp(1 - clip_eps, 1 + clip_eps) * adv
    a_loss_ref = -torch.minimum(l1, l2).mean()
    v_clip = old_value + (vf - old_value).clamp(-clip_eps, clip_eps)
    v_loss_ref = 0.5 * torch.maximum((vf - targets) ** 2, (v_clip - targets) ** 2).mean()
    assert abs(metrics[0].item() - a_loss_ref.item()) < 0.03 * (1 + abs(a_loss_ref.item()))
    assert abs(metrics[1].item() - v_loss_ref.item()) < 0.03 * (1 + abs(v_loss_ref.item()))
    ent = metrics[2].item()
    base_ent = (0.5 * math.log(2 * math.pi * math.e) + sigma.log()).sum(-1).mean().item()
    assert ent < base_ent + 1.0 and ent > base_ent - 2.0 * ACT

    eps_ent = torch.zeros(B, ACT, device=device)
    dloc_ref, dspre_ref, dv_ref = closed_form_grads(
        locf.double(), spref.double(), vf.double(), action.double(),
        old_logp.double(), old_value.double(), adv.double(), targets.double(),
        eps_ent.double(), clip_eps, 0.0, vf_coef, 1e-3, 1.0, 0.0)
    torch.testing.assert_close(dhead.float()[:, 0:ACT], dloc_ref.float(),
                               rtol=5e-2, atol=2e-4)
    torch.testing.assert_close(dhead.float()[:, 8 : 8 + ACT], dspre_ref.float(),
                               rtol=5e-2, atol=2e-4)
    torch.testing.assert_close(dv.view(-1).float(), dv_ref.float(),
                               rtol=5e-2, atol=2e-4)


@requires_gpu
def test_fused_adam_bf16_matches_torch(ext):
    n = 5000
    g = torch.Generator().manual_seed(5)
    p32 = torch.randn(n, generator=g).cuda()
    p_ref = p32.clone()
    grads = [torch.randn(n, generator=g).cuda() for _ in range(5)]
    m = torch.zeros(n).cuda()
    v = torch.zeros(n).cuda()
    sqn = torch.zeros(1).cuda()
    st = torch.zeros(1, dtype=torch.int64).cuda()
    p16 = torch.zeros(n, dtype=torch.bfloat16).cuda()
    lr, max_norm = 3e-4, 0.5
    ref_p = torch.nn.Parameter(p_ref)
    opt = torch.optim.Adam([ref_p], lr=lr, eps=1e-5)
    for gr in grads:
        g16 = gr.bfloat16()
        ext.fused_adam_bf16(p32, g16, m, v, sqn, st, p16, lr, 0.9, 0.999,
                            1e-5, max_norm, 1.0, 1)
        ref_p.grad = g16.float()
        torch.nn.utils.clip_grad_norm_([ref_p], max_norm)
        opt.step()
    torch.cuda.synchronize()
    torch.testing.assert_close(p32, ref_p.detach(), rtol=1e-4, atol=1e-5)
    torch.testing.assert_close(p16.float(), p32, rtol=1e-2, atol=1e-2)


@requires_gpu
def test_fused_adam_bf16_ordered_norm_is_reproducible(ext):
    """With room for per-block partials behind sqnorm[0], the grad norm is
    summed in a fixed order: two runs from the same state are bit-identical,
    exactly the 49 partial slots this size needs are written, sqnorm[0] is
    their sum in the kernel's order (lane-strided, then the shuffle tree),
    and the update still matches torch clip+Adam. n spans 49 norm blocks
    with a tail that is no multiple of the 8-wide vector."""
    n = 100_003
    g = torch.Generator().manual_seed(7)
    p0 = torch.randn(n, generator=g).cuda()
    grads = [torch.randn(n, generator=g).cuda().bfloat16() for _ in range(3)]
    lr, max_norm = 3e-4, 0.5

    def run():
        p32 = p0.clone()
        m = torch.zeros(n).cuda()
        v = torch.zeros(n).cuda()
        sqn = torch.zeros(1 + 2048).cuda()
        st = torch.zeros(1, dtype=torch.int64).cuda()
        p16 = torch.zeros(n, dtype=torch.bfloat16).cuda()
        for g16 in grads:
            ext.fused_adam_bf16(p32, g16, m, v, sqn, st, p16, lr, 0.9, 0.999,
                                1e-5, max_norm, 1.0, 1)
        torch.cuda.synchronize()
        return p32, sqn

    pa, sqa = run()
    pb, sqb = run()
    assert torch.equal(pa, pb)
    assert torch.equal(sqa, sqb)
    # the ordered path ran (not the atomic fallback): one partial per block,
    # blocks = ceil((n // 8) / 256) = 49, nothing written past them
    blocks = (n // 8 + 255) // 256
    assert blocks == 49
    parts = sqa[1 : 1 + blocks].cpu()
    assert (parts > 0).all()
    assert (sqa[1 + blocks :] == 0).all()
    # replay the kernel's order in fp32: lane l takes partials l, l+64, ...
    # (at most one here), then acc[l] += acc[l + off] for off = 32 .. 1
    lanes = torch.zeros(64)
    lanes[:blocks] = parts
    for off in (32, 16, 8, 4, 2, 1):
        lanes[:off] = lanes[:off] + lanes[off : 2 * off]
    assert torch.equal(lanes[0], sqa[0].cpu())
    # fp32 sum of 1e5 squares in short chains + trees: well inside 1e-5
    want = grads[-1].double().pow(2).sum()
    torch.testing.assert_close(sqa[0].double(), want, rtol=1e-5, atol=0.0)

    ref_p = torch.nn.Parameter(p0.clone())
    opt = torch.optim.Adam([ref_p], lr=lr, eps=1e-5)
    for g16 in grads:
        ref_p.grad = g16.float()
        torch.nn.utils.clip_grad_norm_([ref_p], max_norm)
        opt.step()
    torch.testing.assert_close(pa, ref_p.detach(), rtol=1e-4, atol=1e-5)


@requires_gpu
def test_fused_ppo_update_step_runs_and_learns_shape(ext):
    """End-to-end: PPOLearner with the fused engine active — one update
    step runs, metrics finite, and the fused path is actually attached."""
    from stoix_amd import envs as environments
    from stoix_amd.config import compose
    from stoix_amd.systems.ppo.ff_ppo import PPOLearner
    from stoix_amd.utils.total_timestep_checker import check_total_timesteps

    cfg = compose(
        "default/anakin/default_ff_ppo_continuous.yaml",
        [
            "env=brax/ant",
            "arch.total_num_envs=256",
            "arch.total_timesteps=null",
            "arch.num_updates=4",
            "arch.num_evaluation=1",
            "system.rollout_length=16",
            "system.num_minibatches=2",
            "system.epochs=2",
            "system.compute_dtype=bf16",
            "logger.loggers=[]",
        ],
    )
    cfg.arch.n_devices = 1
    check_total_timesteps(cfg)
    device = torch.device("cuda:0")
    env = environments.make_single(cfg, 256, device, seed=0)
    learner = PPOLearner(cfg, env, device)
    assert learner.fused is not None, "fused engine must attach on ant/bf16"
    m1 = learner.update_step()
    m2 = learner.update_step()
    torch.cuda.synchronize()
    for k, val in m2.items():
        assert torch.isfinite(val).all(), f"{k} not finite"
    # params actually moved
    w = learner.fused.actor_chain.flat
    assert w.abs().sum() > 0
    # 2 update calls x 2 epochs x 2 minibatches of Adam steps
    assert learner.fused.actor_chain.step_t.item() == 2 * 2 * 2


@requires_gpu
def test_fused_vs_eager_gradients_one_minibatch(ext):
    """Single-minibatch gradient parity: run ONE fused minibatch update and
    the eager fp32 backward on identical params and identical rollout data
    (ent_coef=0 so the stochastic entropy term has no gradient); the fused
    bf16 gradients must align with the eager fp32 gradients (cosine > 0.98
    and norm ratio within 15%) for every parameter tensor."""
    from stoix_amd import envs as environments
    from stoix_amd.config import compose
    from stoix_amd.systems.ppo.ff_ppo import PPOLearner
    from stoix_amd.utils.total_timestep_checker import check_total_timesteps

    def mk(fused: bool):
        cfg = compose(
            "default/anakin/default_ff_ppo_continuous.yaml",
            [
                "env=brax/ant",
                "arch.total_num_envs=256",
                "arch.total_timesteps=null",
                "arch.num_updates=4",
                "arch.num_evaluation=1",
                "arch.seed=11",
                "system.rollout_length=16",
                "system.num_minibatches=1",
                "system.epochs=1",
                "system.ent_coef=0.0",
                f"system.compute_dtype={'bf16' if fused else 'fp32'}",
                f"system.fused={str(fused).lower()}",
                "logger.loggers=[]",
            ],
        )
        cfg.arch.n_devices = 1
        check_total_timesteps(cfg)
        device = torch.device("cuda:0")
        torch.manual_seed(11)
        env = environments.make_single(cfg, 256, device, seed=3)
        return PPOLearner(cfg, env, device)

    torch.manual_seed(11)
    fused = mk(True)
    assert fused.fused is not None
    torch.manual_seed(11)
    eager = mk(False)
    assert eager.fused is None
    eager.load_params(fused.snapshot_params())

    # identical rollout data: run fused rollout, copy buffers to eager
    fused.rollout_phase()
    for name in ["buf_obs", "buf_action", "buf_log_prob", "buf_value",
                 "buf_bootstrap", "buf_reward", "buf_discount", "buf_adv",
                 "buf_targets"]:
        getattr(eager, name).copy_(getattr(fused, name))
    perm = torch.arange(fused.T * fused.B, device=fused.device)
    fused.perm_buf.copy_(perm)
    eager.perm_buf.copy_(perm)

    # eager: single backward, capture grads (no optimizer step)
    TB = eager.T * eager.B
    import torch.nn.functional as TF
    obs = eager.buf_obs.view(TB, -1)
    act = eager.buf_action.view(TB, -1)
    for p in list(eager.actor.parameters()) + list(eager.critic.parameters()):
        p.grad = None
    dist = eager.actor(obs)
    new_logp = dist.log_prob(act)
    value = eager.critic(obs)
    from stoix_amd.ops.losses import clipped_value_loss, ppo_clip_loss
    a_loss = ppo_clip_loss(new_logp, eager.buf_log_prob.view(TB),
                           eager.buf_adv.view(TB), float(eager.sys.clip_eps))
    v_loss = clipped_value_loss(value, eager.buf_value.view(TB),
                                eager.buf_targets.view(TB),
                                float(eager.sys.clip_eps))
    (a_loss + float(eager.sys.vf_coef) * v_loss).backward()

    # fused: one epoch (1 minibatch) -> grad16 holds that minibatch's grads
    fused.epoch_phase()
    torch.cuda.synchronize()

    F_ = fused.fused
    ag = F_.actor_chain.gviews16
    cg = F_.critic_chain.gviews16
    al = [m for m in eager.actor.torso.net if hasattr(m, "weight")]
    cl = [m for m in eager.critic.torso.net if hasattr(m, "weight")]
    OBS = F_.OBS
    pairs = {
        "a.W1": (ag["W1"][:, :OBS], al[0].weight.grad),
        "a.b1": (ag["b1"], al[0].bias.grad),
        "a.W2": (ag["W2"], al[1].weight.grad),
        "a.b2": (ag["b2"], al[1].bias.grad),
        "a.Wloc": (ag["Wh"][0:8], eager.actor.action_head.loc.weight.grad),
        "a.Wscale": (ag["Wh"][8:16], eager.actor.action_head.scale.weight.grad),
        "c.W1": (cg["W1"][:, :OBS], cl[0].weight.grad),
        "c.W2": (cg["W2"], cl[1].weight.grad),
        "c.Wv": (cg["Wv"], eager.critic.critic_head.linear.weight.grad.view(-1)),
    }
    for name, (gf, ge) in pairs.items():
        gf = gf.float().flatten()
        ge = ge.float().flatten()
        cos = TF.cosine_similarity(gf, ge, dim=0).item()
        ratio = (gf.norm() / ge.norm().clamp_min(1e-12)).item()
        assert cos > 0.98, f"{name}: cosine {cos:.4f}"
        assert 0.85 < ratio < 1.18, f"{name}: norm ratio {ratio:.3f}"


@requires_gpu
@pytest.mark.parametrize("N,K,NV", [(256, 256, 256), (256, 32, 256), (16, 256, 16), (16, 256, 1)])
def test_wgrad_kernel_matches_mm(ext, N, K, NV):
    """Split-K wgrad kernel (wgrad.hip): dW = dZ^T @ X and db = colsum(dZ)
    through the slab + slab_reduce path, vs torch fp32 reference."""
    S = 2048
    g = torch.Generator().manual_seed(9)
    dZ = (torch.randn(S, N, generator=g) * 0.1).bfloat16().cuda()
    X = torch.randn(S, K, generator=g).bfloat16().cuda()
    numel = NV * K + NV
    slab = torch.zeros(64, numel, device="cuda")
    grad16 = torch.zeros(numel, dtype=torch.bfloat16, device="cuda")
    e0 = torch.zeros(0, device="cuda")
    e1 = torch.zeros(0, dtype=torch.int64, device="cuda")
    ext.wgrad(dZ, X, slab, 0, NV * K, NV)
    ext.slab_reduce(slab, grad16, e0, e1)
    torch.cuda.synchronize()
    dW = grad16[: NV * K].view(NV, K).float()
    db = grad16[NV * K :].float()
    ref_w = (dZ.float().t() @ X.float())[:NV]
    ref_b = dZ.float().sum(0)[:NV]
    torch.testing.assert_close(dW, ref_w, rtol=3e-2, atol=3e-2)
    torch.testing.assert_close(db, ref_b, rtol=3e-2, atol=3e-1)
    assert (slab == 0).all()  # reduce re-zeroes for the next minibatch


@requires_gpu
def test_fused_rollout_megakernel_invariants(ext):
    """rollout_step_ant megakernel: stored log-probs/values must agree with
    the eager modules evaluated on the stored observations/actions (the
    module params are fp32 views of the fused masters)."""
    from stoix_amd import envs as environments
    from stoix_amd.config import compose
    from stoix_amd.systems.ppo.ff_ppo import PPOLearner
    from stoix_amd.utils.total_timestep_checker import check_total_timesteps

    cfg = compose(
        "default/anakin/default_ff_ppo_continuous.yaml",
        [
            "env=brax/ant", "arch.total_num_envs=256", "arch.total_timesteps=null",
            "arch.num_updates=4", "arch.num_evaluation=1",
            "system.rollout_length=8", "system.num_minibatches=2",
            "system.epochs=1", "system.compute_dtype=bf16", "logger.loggers=[]",
        ],
    )
    cfg.arch.n_devices = 1
    check_total_timesteps(cfg)
    device = torch.device("cuda:0")
    env = environments.make_single(cfg, 256, device, seed=0)
    learner = PPOLearner(cfg, env, device)
    assert learner.fused is not None
    learner.rollout_phase()
    torch.cuda.synchronize()
    for t in [0, 3, 7]:
        obs = learner.buf_obs[t]
        act = learner.buf_action[t]
        with torch.no_grad():
            dist = learner.actor(obs)
            logp = dist.log_prob(act)
            v = learner.critic(obs)
        torch.testing.assert_close(learner.buf_log_prob[t], logp, rtol=5e-2, atol=0.15)
        torch.testing.assert_close(learner.buf_value[t], v, rtol=5e-2, atol=5e-2)
    # rewards/discounts sane; steptypes valid
    assert torch.isfinite(learner.buf_reward).all()
    assert ((learner.buf_discount == 0) | (learner.buf_discount == 1)).all()
    # bootstrap identity: for non-done rows V(next_obs) == next step's value
    done = learner.fused.buf_steptype >= 2
    nd = ~done[:-1]
    torch.testing.assert_close(
        learner.buf_bootstrap[:-1][nd], learner.buf_value[1:][nd],
        rtol=0, atol=0)
    # for done rows the in-kernel critic supplied V(pre-reset next_obs):
    # finite and in the value range
    assert torch.isfinite(learner.buf_bootstrap).all()


ANT_MAX_STEPS = 1000


def _rollout_step_ant_once(ext, H, ACT=8, truncate_rows=(), with_reference=True):
    """One rollout_step_ant launch on B = 40 freshly reset Ant envs (two
    full 16-row tiles plus one half tile), preceded (`with_reference`) by
    policy_value_step on the same obs, weights, policy seed and draw
    (counter 5 + offset 3). Rows in `truncate_rows` start one step short of
    the episode limit."""
    dev = "cuda"
    B, OBS = 40, 27
    # (weight, bias) pairs: weights go in as bf16 mirrors, biases stay fp32
    w = [t.bfloat16() if i % 2 == 0 else t
         for i, t in enumerate(_mk_weights(H, OBS, ACT, dev))]
    state = torch.zeros(B, 29, device=dev)
    ext.ant_reset(state, 77, 0)
    # obs layout of ant_core.h ant_write_obs (pure copies of state columns)
    obs = torch.cat([state[:, 2:3], state[:, 3:7], state[:, 13:21],
                     state[:, 7:10], state[:, 10:13], state[:, 21:29]], 1).contiguous()
    e = torch.zeros(0, device=dev)
    f = lambda *s: torch.zeros(*s, device=dev)
    i32 = lambda *s: torch.zeros(*s, dtype=torch.int32, device=dev)
    draw = torch.full((1,), 5, dtype=torch.int32, device=dev)
    seed, off = 4321, 3
    ref = dict(obs=f(B, OBS), action=f(B, ACT), logp=f(B), value=f(B))
    if with_reference:
        ext.policy_value_step(obs.clone(), *w, ref["obs"], ref["action"],
                              ref["logp"], ref["value"], e, e, 1e-3, 1.0, 0.0,
                              0.0, 0, seed, draw, off, 0)
    step_count = i32(B)
    step_count[list(truncate_rows)] = ANT_MAX_STEPS - 1
    out = dict(obs=f(B, OBS), action=f(B, ACT), logp=f(B), value=f(B),
               bootstrap=torch.full((B,), float("nan"), device=dev),
               reward=f(B), discount=f(B),
               steptype=torch.zeros(B, dtype=torch.uint8, device=dev))
    ext.rollout_step_ant(
        obs.clone(), state, step_count, f(B), i32(B), f(B), i32(B), *w,
        out["obs"], out["action"], out["logp"], out["value"], out["bootstrap"],
        out["reward"], out["discount"], out["steptype"], ANT_MAX_STEPS, 1e-3,
        1.0, 0.0, 0.0, seed, 99, draw, i32(1), off)
    torch.cuda.synchronize()
    assert draw.item() == 5  # neither call bumps the counter
    return ref, out


@requires_gpu
@pytest.mark.parametrize("H", [128, 256, 512])
def test_rollout_step_ant_matches_policy_value_step(ext, H):
    """The megakernel and policy_value_step share one forward and one
    sampling epilogue: same inputs, seed and draw give bit-equal obs
    mirror, action, log-prob and value at every instantiated width."""
    ref, out = _rollout_step_ant_once(ext, H)
    for k in ("obs", "action", "logp", "value"):
        assert torch.equal(out[k], ref[k]), k


@requires_gpu
@pytest.mark.parametrize("H", [128, 256, 512])
def test_rollout_step_ant_bootstrap_only_on_done_rows(ext, H):
    """The bootstrap critic pass stores V(next_obs) for done rows only (the
    row mask handed to the shared value head): rows 1, 17 and 39 truncate,
    one in each tile, and every row that did not end keeps its NaN fill."""
    rows = (1, 17, 39)
    _, out = _rollout_step_ant_once(ext, H, truncate_rows=rows)
    done = out["steptype"] >= 2
    assert done[list(rows)].all()
    assert not done.all()
    assert torch.isfinite(out["bootstrap"][done]).all()
    assert torch.isnan(out["bootstrap"][~done]).all()


@requires_gpu
def test_fused_mlp_rejects_unsupported_shapes(ext):
    """Widths and head sizes no kernel is instantiated for raise before any
    launch instead of running a kernel of another shape."""
    dev = "cuda"
    B, OBS = 40, 27
    w = _mk_weights(64, OBS, 8, dev)
    bf = lambda t: t.bfloat16()
    e = torch.zeros(0, device=dev)
    obs, v = torch.zeros(B, OBS, device=dev), torch.zeros(B, device=dev)
    with pytest.raises(RuntimeError, match="HID 128/256/512, got 64"):
        ext.value_forward(obs, bf(w[6]), w[7], bf(w[8]), w[9], bf(w[10]),
                          w[11], v, e, e)
    # the messages come from the rollout_step_ant wrapper alone
    with pytest.raises(RuntimeError, match="HID 128/256/512, got 64"):
        _rollout_step_ant_once(ext, 64, with_reference=False)
    with pytest.raises(RuntimeError, match="rollout_step_ant needs OBS == 27 and ACT == 8"):
        _rollout_step_ant_once(ext, 128, ACT=4, with_reference=False)


@requires_gpu
@pytest.mark.parametrize("K", [32, 256])
def test_linear_silu_kernel_matches_torch(ext, K):
    S, N = 2048, 256
    g = torch.Generator().manual_seed(12)
    X = (torch.randn(S, K, generator=g) / math.sqrt(K)).bfloat16().cuda()
    W = (torch.randn(N, K, generator=g) / math.sqrt(K)).bfloat16().cuda()
    b = (torch.randn(N, generator=g) * 0.1).cuda()
    Z = torch.zeros(S, N, dtype=torch.bfloat16, device="cuda")
    H = torch.zeros(S, N, dtype=torch.bfloat16, device="cuda")
    ext.linear_silu(X, W, b, Z, H, 1)
    torch.cuda.synchronize()
    Zref = X.float() @ W.float().t() + b
    torch.testing.assert_close(Z.float(), Zref, rtol=3e-2, atol=3e-2)
    torch.testing.assert_close(H.float(), F.silu(Zref), rtol=3e-2, atol=3e-2)


# --------------------------------------------------- discrete (categorical)


@requires_gpu
@pytest.mark.parametrize("H,OBS,ACT", [(256, 4, 2), (256, 27, 6), (128, 10, 16), (512, 4, 2)])
def test_policy_value_step_disc_matches_eager(ext, H, OBS, ACT):
    """Fused categorical rollout kernel vs plain fp32 eager: value head,
    greedy action = argmax(logits), logp = log_softmax(logits)[a]."""
    dev = "cuda"
    W1a, b1a, W2a, b2a, _, _, W1c, b1c, W2c, b2c, Wvc, bvc = _mk_weights(
        H, OBS, min(ACT, 8), dev
    )
    # categorical packing: logits rows 0..ACT-1 of the 16-row tile
    g = torch.Generator().manual_seed(11)
    Wha = torch.zeros(16, H, device=dev)
    Wha[0:ACT] = torch.randn(ACT, H, generator=g).to(dev) / math.sqrt(H)
    bha = torch.zeros(16, device=dev)
    bha[0:ACT] = torch.randn(ACT, generator=g).to(dev) * 0.1
    B = 977
    obs = torch.randn(B, OBS, generator=g).to(dev)
    action = torch.zeros(B, dtype=torch.long, device=dev)
    logp = torch.zeros(B, device=dev)
    value = torch.zeros(B, device=dev)
    empty = torch.zeros(0, device=dev)
    mirror = torch.zeros(B, OBS, device=dev)
    ext.policy_value_step_disc(
        obs, W1a.bfloat16(), b1a, W2a.bfloat16(), b2a, Wha.bfloat16(), bha,
        W1c.bfloat16(), b1c, W2c.bfloat16(), b2c, Wvc.bfloat16(), bvc,
        mirror, action, logp, value, empty, empty,
        ACT, 1, 123, torch.zeros(0, dtype=torch.int32, device=dev), 0, 0,
    )
    ha = _eager_forward(obs, W1a, b1a, W2a, b2a)
    hc = _eager_forward(obs, W1c, b1c, W2c, b2c)
    logits = F.linear(ha, Wha[:ACT], bha[:ACT])
    v_ref = F.linear(hc, Wvc.view(1, -1), bvc).view(-1)
    a_ref = logits.argmax(-1)
    lp_ref = F.log_softmax(logits, dim=-1).gather(1, a_ref.unsqueeze(1)).squeeze(1)
    torch.testing.assert_close(mirror, obs)
    assert (action == a_ref).float().mean() > 0.99  # bf16 argmax ties only
    match = action == a_ref
    torch.testing.assert_close(logp[match], lp_ref[match], rtol=5e-2, atol=5e-2)
    torch.testing.assert_close(value, v_ref, rtol=5e-2, atol=5e-2)


@requires_gpu
def test_policy_value_step_disc_sampling_statistics(ext):
    """Gumbel-max sampling frequencies match softmax probabilities."""
    dev = "cuda"
    H, OBS, ACT = 256, 4, 4
    W1a, b1a, W2a, b2a, Wha, bha, W1c, b1c, W2c, b2c, Wvc, bvc = _mk_weights(
        H, OBS, ACT, dev
    )
    Wha.zero_(); Wha[0:ACT] = 0.0
    bha.zero_()
    bha[0:ACT] = torch.tensor([0.0, 1.0, 2.0, -1.0], device=dev)
    B = 200_000
    obs = torch.zeros(B, OBS, device=dev)
    action = torch.zeros(B, dtype=torch.long, device=dev)
    logp = torch.zeros(B, device=dev)
    value = torch.zeros(B, device=dev)
    empty = torch.zeros(0, device=dev)
    ext.policy_value_step_disc(
        obs, W1a.bfloat16(), b1a, W2a.bfloat16(), b2a, Wha.bfloat16(), bha,
        W1c.bfloat16(), b1c, W2c.bfloat16(), b2c, Wvc.bfloat16(), bvc,
        torch.zeros(0, device=dev), action, logp, value, empty, empty,
        ACT, 0, 987, torch.zeros(0, dtype=torch.int32, device=dev), 0, 0,
    )
    p_ref = F.softmax(bha[0:ACT], dim=-1)
    counts = torch.bincount(action, minlength=ACT).float() / B
    assert (counts - p_ref).abs().max().item() < 0.01, (counts, p_ref)
    # logp of the sampled action matches log_softmax
    lp_ref = F.log_softmax(bha[0:ACT], dim=-1)[action]
    torch.testing.assert_close(logp, lp_ref, rtol=2e-2, atol=2e-2)


@requires_gpu
def test_ppo_head_loss_disc_matches_autograd(ext):
    """Categorical PPO head loss + analytic logits/value grads vs a full
    autograd fp32 reference."""
    dev = "cuda"
    ACT, B = 6, 4096
    g = torch.Generator().manual_seed(3)
    logits16 = torch.zeros(B, 16, device=dev)
    logits16[:, :ACT] = torch.randn(B, ACT, generator=g).to(dev)
    v_in = torch.randn(B, generator=g).to(dev)
    action = torch.randint(0, ACT, (B,), generator=g).to(dev)
    old_logp = (torch.randn(B, generator=g) * 0.2 - 1.5).to(dev)
    old_value = torch.randn(B, generator=g).to(dev)
    adv = torch.randn(B, generator=g).to(dev)
    targets = torch.randn(B, generator=g).to(dev)
    clip_eps, ent_coef, vf_coef = 0.2, 0.01, 0.5

    dhead = torch.zeros(B, 16, dtype=torch.bfloat16, device=dev)
    dv = torch.zeros(B, dtype=torch.bfloat16, device=dev)
    dv16 = torch.zeros(B, 16, dtype=torch.bfloat16, device=dev)
    metrics = torch.zeros(3, device=dev)
    ext.ppo_head_loss_disc(
        logits16.bfloat16(), v_in.bfloat16(), action, old_logp, old_value,
        adv, targets, dhead, dv, dv16, metrics, ACT, clip_eps, ent_coef,
        vf_coef,
    )

    # autograd reference (stoix_amd.ops.losses semantics)
    from stoix_amd.ops.losses import clipped_value_loss, ppo_clip_loss

    lg = logits16[:, :ACT].clone().requires_grad_(True)
    vv = v_in.clone().requires_grad_(True)
    dist_logp = F.log_softmax(lg, dim=-1)
    new_logp = dist_logp.gather(1, action.unsqueeze(1)).squeeze(1)
    entropy = -(dist_logp.exp() * dist_logp).sum(-1).mean()
    a_loss = ppo_clip_loss(new_logp, old_logp, adv, clip_eps)
    v_loss = clipped_value_loss(vv, old_value, targets, clip_eps)
    total = a_loss - ent_coef * entropy + vf_coef * v_loss
    total.backward()

    torch.testing.assert_close(metrics[0], a_loss.detach(), rtol=2e-2, atol=2e-2)
    torch.testing.assert_close(metrics[1], v_loss.detach(), rtol=2e-2, atol=2e-2)
    torch.testing.assert_close(metrics[2], entropy.detach(), rtol=2e-2, atol=2e-2)
    torch.testing.assert_close(dhead.float()[:, :ACT], lg.grad, rtol=5e-2, atol=5e-3)
    assert (dhead.float()[:, ACT:] == 0).all()
    torch.testing.assert_close(dv.float(), vv.grad, rtol=5e-2, atol=5e-3)


@requires_gpu
def test_fused_discrete_cartpole_update_runs(ext):
    """End-to-end: discrete CartPole PPO builds the fused engine and steps;
    losses stay finite and the policy logits move."""
    from stoix_amd import envs as environments
    from stoix_amd.config import compose
    from stoix_amd.systems.ppo.ff_ppo import PPOLearner
    from stoix_amd.utils.total_timestep_checker import check_total_timesteps

    cfg = compose(
        "default/anakin/default_ff_ppo.yaml",
        ["env=classic/cartpole", "arch.total_num_envs=2048",
         "arch.total_timesteps=null", "arch.num_updates=4",
         "arch.num_evaluation=1", "system.rollout_length=16",
         "system.num_minibatches=4", "system.epochs=2",
         "system.compute_dtype=bf16", "logger.loggers=[]"],
    )
    cfg.arch.n_devices = 1
    check_total_timesteps(cfg)
    dev = torch.device("cuda:0")
    env = environments.make_single(cfg, 2048, dev, seed=3)
    learner = PPOLearner(cfg, env, dev)
    assert learner.fused is not None and learner.fused.discrete
    w_before = learner.actor.action_head.linear.weight.detach().clone()
    for _ in range(3):
        m = learner.update_step()
    torch.cuda.synchronize()
    for v in m.values():
        assert torch.isfinite(v).all()
    w_after = learner.actor.action_head.linear.weight.detach()
    assert (w_after - w_before).abs().max() > 0


@requires_gpu
def test_fused_obs_norm_cartpole(ext):
    """Fused engine with observation normalisation: stats update in place
    each rollout, the trajectory is normalised with PRE-update stats, and
    the update stays finite (reference ff_ppo.py:90-162 path)."""
    from stoix_amd import envs as environments
    from stoix_amd.config import compose
    from stoix_amd.systems.ppo.ff_ppo import PPOLearner
    from stoix_amd.utils.total_timestep_checker import check_total_timesteps

    cfg = compose(
        "default/anakin/default_ff_ppo.yaml",
        ["env=classic/cartpole", "arch.total_num_envs=1024",
         "arch.total_timesteps=null", "arch.num_updates=4",
         "arch.num_evaluation=1", "system.rollout_length=16",
         "system.num_minibatches=4", "system.epochs=2",
         "system.compute_dtype=bf16", "system.normalize_observations=true",
         "logger.loggers=[]"],
    )
    cfg.arch.n_devices = 1
    check_total_timesteps(cfg)
    dev = torch.device("cuda:0")
    env = environments.make_single(cfg, 1024, dev, seed=3)
    learner = PPOLearner(cfg, env, dev)
    assert learner.normalize_obs
    assert learner.fused is not None and learner.fused.norm
    # capture the phases too: the Welford update runs INSIDE the rollout
    # graph (a capture-illegal op here once shipped behind the uncaptured
    # version of this test)
    from stoix_amd.ops.graph import try_enable_graphs

    assert try_enable_graphs(learner)
    c0 = float(learner.obs_stats.count)
    for _ in range(3):
        m = learner.update_step()
    torch.cuda.synchronize()
    for v in m.values():
        assert torch.isfinite(v).all()
    # Welford state advanced by T*B per rollout, in place
    assert float(learner.obs_stats.count) == c0 + 3 * 16 * 1024
    assert float(learner.obs_stats.std.min()) > 0
    # stats are no longer the init values (mean moved)
    assert float(learner.obs_stats.mean.abs().sum()) > 0
