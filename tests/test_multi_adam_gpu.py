"""GPU tests of the multi-tensor optimiser tail (ops/csrc/multi_adam.hip)
through ``OptimTail.step`` on real ``torch.optim.Adam(capturable=True)``.

Reference: the formulas of multi_adam.hip in float64 on the CPU, on the
float32-rounded values the arithmetic consumes (b, 1 - b, lr, eps, tau,
1 - tau, max_norm), ``max_norm`` at 0.37x (clip active) or 2x (inactive) the
float64 norm. Tolerance: the same tensors go through the torch calls in fp32
(the chain, ``STOIX_FUSED_OPTIM=0``); per chain and for each of the applied
update, ``exp_avg``, ``exp_avg_sq`` and the target, ``max|fused - fp64| <=
2 max|chain - fp64| + 1 fp32 ulp`` of the largest magnitude; every ``step``
equals the float64 ``t``. Worst ``err / (2 err_chain + ulp)`` seen: 0.638.
"""
import math

import numpy as np
import pytest
import torch
import torch.nn as nn

pytestmark = pytest.mark.gpu

requires_gpu = pytest.mark.skipif(not torch.cuda.is_available(), reason="no GPU")

B1, B2, LR, TAU = 0.9, 0.999, 3e-4, 0.005
# "view": base[1:] of a larger tensor (4-byte aligned); "nograd": grad = None
SIZES = [(), (1,), (51,), (2047,), (2048,), (2049,), (3, 1500), "view", "nograd"]
KEYS = ("p", "m", "v", "tgt")


def f32(x):
    return float(np.float32(x))


def _chain(seed, clip, target, eps, step0, sizes=SIZES):
    g = torch.Generator().manual_seed(seed)
    r = lambda shape, scale=1.0: torch.randn(shape, generator=g) * scale
    ts = []
    for kind in sizes:
        s = (51,) if isinstance(kind, str) else kind
        ts.append({"kind": kind, "p": r(s), "g": r(s, 0.01), "tgt": r(s),
                   "m": r(s, 0.01) if step0 else torch.zeros(s),
                   "v": r(s, 0.01).square() if step0 else torch.zeros(s)})
    norm = math.sqrt(sum(float(t["g"].double().square().sum()) for t in ts if t["kind"] != "nograd"))
    max_norm = {"active": 0.37 * norm, "inactive": 2.0 * norm, None: None}[clip]
    return {"ts": ts, "max_norm": max_norm, "target": target, "eps": eps, "step0": step0}


def _three(eps, step0):
    """Clip active + polyak, clip inactive + polyak, no clip (a 0-dim log_alpha)."""
    return [_chain(1, "active", True, eps, step0), _chain(2, "inactive", True, eps, step0, SIZES[2:5]),
            _chain(3, None, False, eps, step0, [()])]


def _grad(t, k):
    """Call k's fp32 gradient; the clip branch stays where call 0 has it."""
    return t["g"] * (-0.8) ** k


def _set_grads(chains, tail, k):
    for ch, oc in zip(chains, tail.chains):
        for t, p in zip(ch["ts"], oc.params):
            g = _grad(t, k)
            g = torch.cat([torch.zeros(1), g]).cuda()[1:] if t["kind"] == "view" else g.cuda()
            p.grad = None if t["kind"] == "nograd" else g


def _build(chains):
    from stoix_amd.ops.optim import OptimChain, OptimTail

    out = []
    for ch in chains:
        params, tgts = [], []
        for t in ch["ts"]:
            view = t["kind"] == "view"
            params.append(nn.Parameter(torch.cat([torch.zeros(1), t["p"]]).cuda()[1:] if view else t["p"].cuda()))
            tgts.append(t["tgt"].cuda())
        lr = torch.tensor(LR, device="cuda") if ch["eps"] == 1e-5 else LR  # a tensor lr is read on the device
        opt = torch.optim.Adam(params, lr=lr, eps=ch["eps"], capturable=True)
        if ch["step0"]:  # else the tail creates the state
            for p, t in zip(params, ch["ts"]):
                opt.state[p] = {"step": torch.tensor(float(ch["step0"]), device="cuda"),
                                "exp_avg": t["m"].cuda(), "exp_avg_sq": t["v"].cuda()}
        out.append(OptimChain(opt, params, ch["max_norm"], tgts if ch["target"] else None, TAU))
    return OptimTail(out)


def _run(monkeypatch, chains, knob, calls, active=None, no_sync=False):
    """-> per chain {p, m, v, tgt, step: [cpu tensor or None per tensor]}."""
    monkeypatch.setenv("STOIX_FUSED_OPTIM", knob)
    tail = _build(chains)
    for k in range(calls):
        _set_grads(chains, tail, k)
        torch.cuda.synchronize()
        torch.cuda.set_sync_debug_mode("error" if no_sync else "default")
        try:
            assert tail.step(active) == (knob == "1")
        finally:
            torch.cuda.set_sync_debug_mode("default")
    out = []
    for oc in tail.chains:
        st = [oc.opt.state.get(p, {}) for p in oc.params]
        cpu = lambda xs: [None if x is None else x.detach().cpu() for x in xs]
        out.append({"p": cpu(oc.params), "tgt": cpu(oc.target or []), "m": cpu(s.get("exp_avg") for s in st),
                    "v": cpu(s.get("exp_avg_sq") for s in st), "step": cpu(s.get("step") for s in st)})
    return out


def _reference(ch, calls):
    b1, omb1, b2, omb2, lr, eps, tau, omt = map(f32, (B1, 1 - B1, B2, 1 - B2, LR, ch["eps"], TAU, 1 - TAU))
    ts = [{k: t[k].double().clone() for k in ("p", "m", "v", "tgt")} for t in ch["ts"]]
    live = [t["kind"] != "nograd" for t in ch["ts"]]
    for k in range(calls):
        gs = [_grad(t, k).double() if on else None for t, on in zip(ch["ts"], live)]
        coef = 1.0
        if ch["max_norm"] is not None:
            norm = math.sqrt(sum(float(g.square().sum()) for g in gs if g is not None))
            coef = min(1.0, f32(ch["max_norm"]) / (norm + f32(1e-6)))
        step = ch["step0"] + k + 1
        for t, g in zip(ts, gs):
            if g is not None:
                g = g * coef
                t["m"] += omb1 * (g - t["m"])
                t["v"] = b2 * t["v"] + omb2 * g * g
                t["p"] -= (lr / (1 - b1 ** step)) * t["m"] / (t["v"].sqrt() / math.sqrt(1 - b2 ** step) + eps)
            t["tgt"] = t["tgt"] * omt + tau * t["p"]
    return ts, live, ch["step0"] + calls


def _flat(xs, keep):
    return torch.cat([x.double().reshape(-1) for x, on in zip(xs, keep) if on])


@requires_gpu
@pytest.mark.parametrize("eps,step0,calls,active", [
    (1e-8, 0, 1, None), (1e-5, 999, 1, None), (1e-8, 0, 2, None), (1e-5, 999, 2, (True, False, True)),
])
def test_tail_matches_fp64(monkeypatch, eps, step0, calls, active):
    chains = _three(eps, step0)
    fused = _run(monkeypatch, chains, "1", calls, active)
    chain = _run(monkeypatch, chains, "0", calls, active)
    for c, ch in enumerate(chains):
        if active is not None and not active[c]:  # bit-unchanged, state included
            for t, p, m, v, tg, s in zip(ch["ts"], *(fused[c][k] for k in KEYS + ("step",))):
                assert all(torch.equal(x, t[k]) for x, k in zip((p, m, v, tg), KEYS))
                assert float(s) == step0
            continue
        ref, live, step = _reference(ch, calls)
        assert all(float(s) == step for s, on in zip(fused[c]["step"], live) if on)
        assert all(s is None or float(s) == step0 for s, on in zip(fused[c]["step"], live) if not on)
        for key in KEYS if ch["target"] else KEYS[:3]:
            keep = [True] * len(live) if key in ("p", "tgt") else live
            want = _flat([r[key] for r in ref], keep)
            base = _flat([t["p"] for t in ch["ts"]], keep) if key == "p" else 0.0  # the applied update
            err = [(_flat(run[c][key], keep) - want).abs().max().item() for run in (fused, chain)]
            ulp = float(np.spacing(np.float32((want - base).abs().max().item())))
            print(f"chain {c} {key}: fused {err[0]:.3e} chain {err[1]:.3e} ulp {ulp:.3e} "
                  f"ratio {err[0] / (2 * err[1] + ulp):.3f}")
            assert err[0] <= 2 * err[1] + ulp, (c, key)


@requires_gpu
def test_two_runs_are_bit_equal_without_host_sync(monkeypatch):
    chains = _three(1e-8, 999)
    first = _run(monkeypatch, chains, "1", 1)
    second = _run(monkeypatch, chains, "1", 1, no_sync=True)
    for a, b in zip(first, second):
        assert all(torch.equal(x, y) for k in KEYS + ("step",) for x, y in zip(a[k], b[k]) if x is not None)


@requires_gpu
def test_65_tensors_are_ineligible_and_run_the_torch_calls(monkeypatch):
    chains = [_chain(4, "active", True, 1e-8, 0, [(3,)] * 65)]
    monkeypatch.setenv("STOIX_FUSED_OPTIM", "1")
    tail = _build(chains)
    _set_grads(chains, tail, 0)
    assert tail.step() is False
    want = _run(monkeypatch, chains, "0", 1)[0]
    assert all(torch.equal(p.detach().cpu(), w) for p, w in zip(tail.chains[0].params, want["p"]))
    assert all(torch.equal(x.cpu(), w) for x, w in zip(tail.chains[0].target, want["tgt"]))


@requires_gpu
def test_graph_replays_equal_eager_calls(monkeypatch):
    monkeypatch.setenv("STOIX_FUSED_OPTIM", "1")
    chains = _three(1e-5, 0)
    tails = [_build(chains), _build(chains)]
    for tail in tails:
        _set_grads(chains, tail, 0)
        assert tail.step()  # creates the state; the graph holds these addresses
    for _ in range(2):
        tails[0].step()
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        tails[1].step()
    graph.replay()
    graph.replay()
    torch.cuda.synchronize()
    for a, b in zip(tails[0].chains, tails[1].chains):
        for p, q in zip(a.params, b.params):
            assert torch.equal(p, q)
            for k in a.opt.state.get(p, {}):
                assert torch.equal(a.opt.state[p][k], b.opt.state[q][k]), k
        assert all(torch.equal(x, y) for x, y in zip(a.target or [], b.target or []))


@requires_gpu
def test_sac_learner_steps_with_the_tail_and_hands_its_state_over(monkeypatch):
    from stoix_amd import envs as environments
    from stoix_amd.config import compose
    from stoix_amd.systems.anakin import default_aux_state, load_default_aux_state
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
    one, zero = (SACLearner(cfg, environments.make_single(cfg, 64, dev, seed=0), dev) for _ in range(2))
    monkeypatch.setenv("STOIX_FUSED_OPTIM", "1")
    q_target0 = [p.clone() for p in one.q_target.parameters()]
    for _ in range(2):
        one.update_step()
    for opt in (one.actor_opt, one.q_opt, one.alpha_opt):
        steps = [float(opt.state[p]["step"]) for g in opt.param_groups for p in g["params"]]
        assert steps and all(s == 2.0 for s in steps)
    assert one.tail._partials is not None  # the kernels ran, not the torch calls
    assert all(not torch.equal(a, b) for a, b in zip(q_target0, one.q_target.parameters()))
    monkeypatch.setenv("STOIX_FUSED_OPTIM", "0")
    load_default_aux_state(zero, default_aux_state(one))
    metrics = zero.update_step()
    assert all(math.isfinite(float(v)) for v in metrics.values())
    assert float(zero.q_opt.state[zero.q_opt.param_groups[0]["params"][0]]["step"]) == 3.0
