"""GPU tests of the SAC kernels (ops/csrc/tanh_normal.hip) against today's
torch formulas evaluated in fp64 on the CPU.

Tolerance, fp32 outputs: ``max|kernel - fp64|`` may not exceed twice
``max|torch fp32 chain - fp64|`` on the same inputs plus one fp32 ulp of the
output's largest magnitude (the chain's error can be exactly zero at B = 1).
bf16 outputs lie within one bf16 ulp of the fp64 result rounded to bf16.
"""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

requires_gpu = pytest.mark.skipif(not torch.cuda.is_available(), reason="no GPU")


def _within(name, got, ref, chain):
    """The fp32 rule of the module docstring; prints the figures first."""
    got, err_chain = got.detach().cpu().double(), (chain.double() - ref).abs().max().item()
    err, ulp = (got - ref).abs().max().item(), float(np.spacing(np.float32(ref.abs().max().item())))
    print(f"{name}: kernel {err:.3e} chain {err_chain:.3e} ulp {ulp:.3e}")
    assert got.shape == ref.shape and err <= 2 * err_chain + ulp, name


def _within_bf16(name, got, ref):
    assert got.dtype == torch.bfloat16 and got.shape == ref.shape
    ulp = 2.0 ** (torch.floor(torch.log2(ref.abs().clamp_min(1e-30))) - 7)
    err = (got.detach().cpu().double() - ref.bfloat16().double()).abs()
    print(f"{name}: worst error / bf16 ulp {(err / ulp).max().item():.3f}")
    assert (err <= ulp).all(), name


@requires_gpu
@pytest.mark.parametrize("bounds", [(-1.0, 1.0), (-0.4, 2.0)])
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("B", [1, 5, 257])
@pytest.mark.parametrize("A", [1, 3, 8, 17, 64])
def test_rsample_fwd_bwd_matches_fp64(A, B, dtype, bounds):
    from stoix_amd.networks.distributions import AffineTanhTransformedDistribution as Dist
    from stoix_amd.networks.distributions import _TanhNormalRsample

    g = torch.Generator().manual_seed(1000 * A + B)
    loc = (torch.rand(B, A, generator=g) * 16 - 8).to(dtype)
    scale = (torch.rand(B, A, generator=g) * (2 - 1e-3) + 1e-3).to(dtype)
    eps = torch.randn(B, A, generator=g).clamp(-4, 4)
    da = torch.randn(B, A, generator=g).to(dtype)
    dlogp = torch.randn(B, 2, generator=g)[:, 0]  # element stride 2
    out = {}  # today's formulas on the CPU, in fp64 (reference) and fp32 (chain)
    for cd in (torch.float64, torch.float32):
        lc, sc = (t.to(cd).requires_grad_(True) for t in (loc, scale))
        d = Dist(lc, sc, *bounds)
        u = lc + sc * eps.to(cd)
        a, lp = d._forward(u), d._log_prob_from_u(u)
        grads = torch.autograd.grad([a, lp], [lc, sc], [da.to(cd), dlogp.to(cd)])
        out[cd] = [t.detach() for t in (a, lp, *grads)]
        assert all(torch.isfinite(t).all() for t in out[cd])
    ref, chain = out[torch.float64], out[torch.float32]
    loc, scale = (t.cuda().requires_grad_(True) for t in (loc, scale))
    sa, sh = (bounds[1] - bounds[0]) / 2.0, (bounds[1] + bounds[0]) / 2.0
    a, lp = _TanhNormalRsample.apply(loc, scale, eps.cuda(), sa, sh, True)
    dlogp_dev = torch.empty(B, 2, device="cuda")[:, 0].copy_(dlogp)  # strided too
    got = (a, lp, *torch.autograd.grad([a, lp], [loc, scale], [da.cuda(), dlogp_dev]))
    assert lp.dtype == torch.float32 and a.dtype == got[2].dtype == got[3].dtype == dtype
    for name, k, r, c in zip(("a", "logp", "dloc", "dscale"), got, ref, chain):
        if dtype == torch.bfloat16 and name != "logp":
            _within_bf16(name, k, r)
        else:
            _within(name, k, r, c)


@requires_gpu
def test_rsample_public_route_is_deterministic_and_a65_falls_back(monkeypatch):
    from stoix_amd import ops
    from stoix_amd.networks.distributions import AffineTanhTransformedDistribution as Dist
    from stoix_amd.networks.distributions import _TanhNormalRsample

    monkeypatch.delenv("STOIX_FUSED_SAC", raising=False)

    def gen():
        return torch.Generator(device="cuda").manual_seed(5)

    for A, routed in ((17, True), (65, False)):
        loc = torch.linspace(-3, 3, 257 * A, device="cuda").reshape(257, A).requires_grad_(True)
        scale = torch.full_like(loc, 0.3)
        d = Dist(loc, scale, -0.4, 2.0)
        assert d._route_to_kernel() == routed
        runs = []
        for _ in range(2):
            a, lp = d.sample_and_log_prob(gen())
            runs.append((a, lp, *torch.autograd.grad(lp.sum() + a.sum(), [loc])))
        assert all(torch.equal(x, y) for x, y in zip(*runs))
        eps = torch.randn(loc.shape, device="cuda", generator=gen())
        if routed:  # the public call is the Function on the draw rsample makes
            want = _TanhNormalRsample.apply(loc, scale, eps, d.scale_affine, d.shift_affine, True)
            ext, t_sizes = ops.ext(required=True), []
            fwd = ext.tanh_normal_rsample_fwd
            monkeypatch.setattr(  # record the size of the t each forward is handed
                ext, "tanh_normal_rsample_fwd", lambda *args: (t_sizes.append(args[5].numel()), fwd(*args))[1]
            )
            d.sample_and_log_prob(gen())
            with torch.no_grad():  # t is neither allocated nor stored: same values
                quiet = d.sample_and_log_prob(gen())
            monkeypatch.setattr(ext, "tanh_normal_rsample_fwd", fwd)
            assert t_sizes == [257 * A, 0]
            assert all(torch.equal(x, y) for x, y in zip(quiet, want))
        else:  # today's chain
            u = loc + scale * eps
            want = (d._forward(u), d._log_prob_from_u(u))
        assert all(torch.equal(x, y) for x, y in zip(runs[0][:2], want))
        monkeypatch.setenv("STOIX_FUSED_SAC", "0")
        assert not d._route_to_kernel()
        monkeypatch.delenv("STOIX_FUSED_SAC")


@requires_gpu
@pytest.mark.parametrize("B", [1, 257])
@pytest.mark.parametrize("Q", [1, 2])
def test_sac_losses_match_fp64_composition(Q, B):
    from stoix_amd.ops import losses as L

    g = torch.Generator().manual_seed(10 * Q + B)
    q_pred, q_next, q_new = (torch.randn(Q, B, generator=g) * 3 for _ in range(3))
    q_new[1:, ::3] = q_new[0, ::3]  # ties between the critics (Q = 2)
    q_next[1:, ::3] = q_next[0, ::3]
    logp_next, logp_new = (torch.randn(B, generator=g) * 5 for _ in range(2))
    rd = torch.rand(B, 2, generator=g)  # r and d are its columns, not contiguous
    gamma, h_target = 0.99, -3.0

    def run(dev, cd):
        to = lambda t: t.to(dev, cd, copy=True)  # noqa: E731
        la = torch.tensor(-0.7, device=dev, dtype=cd, requires_grad=True)
        qp, qn, lpn = (to(t).requires_grad_(True) for t in (q_pred, q_new, logp_new))
        rd_d = to(rd)
        q_loss, target = L.sac_critic_loss(
            qp, to(q_next), to(logp_next), rd_d[:, 0], rd_d[:, 1], la, gamma
        )
        actor, dual, ent = L.sac_actor_alpha_losses(qn, lpn, la, h_target)
        (q_loss + 0.5 * actor + 0.25 * dual).backward()
        return dict(q_loss=q_loss, target=target, actor=actor, dual=dual, entropy=ent,
                    dq_pred=qp.grad, dq_new=qn.grad, dlogp_new=lpn.grad, dlog_alpha=la.grad)

    ref, chain, got = run("cpu", torch.float64), run("cpu", torch.float32), run("cuda", torch.float32)
    rows_fn = got["q_loss"].grad_fn.next_functions[0][0].next_functions[0][0]  # div <- mean <- rows
    assert "_SACCriticRows" in type(rows_fn).__name__, "the GPU call did not reach the kernels"
    for name in ref:
        _within(name, got[name], ref[name].detach(), chain[name].detach())
    if Q == 2:  # the tie's gradient goes to critic 0, as torch.min sends it
        dq = got["dq_new"].cpu()
        assert (dq[1, ::3] == 0).all() and (dq[0, ::3] == -(torch.tensor(0.5) / B)).all()


@requires_gpu
def test_sac_update_step_knob_on_matches_knob_off_without_host_sync(monkeypatch):
    """One SACLearner.update_step (one epoch) from identical state and seed,
    three times: knob 0, knob 1, and knob 0 with the float reduction order
    perturbed (the replay batch rows permuted and the rsample noise permuted
    with them, so every row computes what it computed and only the order of the
    sums over the batch changes). Comparison used: per group, the gradients
    handed to the optimiser and the parameters after it may differ between
    knob 0 and knob 1 by at most 4 times (gradients) and 8 times (parameters:
    Adam's first step ``lr * g / (|g| + eps)`` magnifies last bits of near-zero
    gradients) what knob 0 and its perturbed run differ by, plus one fp32 ulp
    of the group's largest magnitude. Values seen on an MI355X are in
    profiles/sac_fused_SUMMARY.md. The fused update then runs a second step
    under sync-debug mode "error": no host synchronisation."""
    from stoix_amd import envs as environments
    from stoix_amd.config import compose
    from stoix_amd.networks.distributions import Normal
    from stoix_amd.systems.sac.ff_sac import SACLearner
    from stoix_amd.utils.total_timestep_checker import check_total_timesteps

    cfg = compose(
        "default/anakin/default_ff_sac.yaml",
        ["env=brax/humanoid", "arch.total_num_envs=64", "arch.total_timesteps=null",
         "arch.num_updates=2", "arch.num_evaluation=1", "system.rollout_length=2",
         "system.batch_size=64", "system.buffer_size=2048", "system.warmup_steps=16",
         "system.epochs=1", "logger.loggers=[]", "logger.checkpointing.save_model=false"],
    )
    cfg.arch.n_devices = 1
    check_total_timesteps(cfg)
    dev = torch.device("cuda:0")
    perm = torch.randperm(64, generator=torch.Generator().manual_seed(2)).to(dev)
    groups = ("actor", "q_online", "q_target")
    rsample = Normal.rsample
    learners, metrics, grads, params = {}, {}, {}, {}
    for run, knob in (("0", "0"), ("1", "1"), ("0 permuted", "0")):
        monkeypatch.setenv("STOIX_FUSED_SAC", knob)
        torch.manual_seed(0)
        learner = learners[run] = SACLearner(cfg, environments.make_single(cfg, 64, dev, seed=0), dev)
        learner.prepare_for_graph_capture()  # device RNG, no host-side metric reads
        if run == "0 permuted":
            sample = learner.buffer.sample
            learner.buffer.sample = lambda n: {k: v[perm] for k, v in sample(n).items()}
            monkeypatch.setattr(Normal, "rsample", lambda self, generator=None: self.loc + self.scale * torch.randn(
                self.loc.shape, device=self.loc.device, generator=generator)[perm])
        reduce = learner.reducer.reduce

        def keep_grads_then_reduce(learner=learner, run=run, reduce=reduce):
            grads[run] = {g: torch.cat([p.grad.flatten() for p in getattr(learner, g).parameters()])
                          for g in groups[:2]}
            grads[run]["log_alpha"] = learner.log_alpha.grad.reshape(1).clone()
            return reduce()

        learner.reducer.reduce = keep_grads_then_reduce
        torch.manual_seed(1)
        metrics[run] = learner.update_step()
        learner.reducer.reduce = reduce
        monkeypatch.setattr(Normal, "rsample", rsample)
        params[run] = {g: torch.cat([p.detach().flatten() for p in getattr(learner, g).parameters()])
                       for g in groups}
        params[run]["log_alpha"] = learner.log_alpha.detach().reshape(1)
    for what, kind, factor in ((grads, "gradient", 4), (params, "parameter", 8)):
        for g in what["0"]:
            seen = (what["1"][g] - what["0"][g]).abs().max().item()
            perturbed = (what["0 permuted"][g] - what["0"][g]).abs().max().item()
            ulp = float(np.spacing(np.float32(what["0"][g].abs().max().item())))
            print(f"{g} {kind}: |knob 1 - knob 0| {seen:.3e}, |permuted - knob 0| {perturbed:.3e}, ulp {ulp:.3e}")
            assert seen <= factor * perturbed + ulp, (g, kind)
    for k in ("q_loss", "actor_loss", "entropy"):
        torch.testing.assert_close(metrics["1"][k], metrics["0"][k], rtol=1e-4, atol=1e-4)
    torch.cuda.synchronize()
    monkeypatch.setenv("STOIX_FUSED_SAC", "1")
    torch.cuda.set_sync_debug_mode("error")
    try:
        learners["1"].update_step()
    finally:
        torch.cuda.set_sync_debug_mode("default")
    torch.cuda.synchronize()
