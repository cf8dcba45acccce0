"""GPU tests of the Q-ensemble layer kernels (ops/csrc/qens.hip) against plain
fp64 torch on the CPU.

Kernel bounds, per element, for a sum of L fp32 products in any order:
``|got - ref64| <= (L + c) * 2^-24 * sum |terms|``, the terms taken in fp64.
Forward: L = K0 + K1, c = 3 (bias add), and for H ``1.1 * bound_Z + 2^-21 |H|``
(|silu'| < 1.1; an exp, an add and a divide). Backward: c = 16 for forming
``dZ = dH * act'``; L = N (dgrad), E * N (dgrad summed over members), S (wgrad,
db). The module-level test uses the rule of tests/test_sac_fused_gpu.py:
``max|fused - fp64| <= 2 max|fp32 chain - fp64| + 1 fp32 ulp``.
"""
import copy

import numpy as np
import pytest
import torch
import torch.nn as nn

pytestmark = pytest.mark.gpu

requires_gpu = pytest.mark.skipif(not torch.cuda.is_available(), reason="no GPU")

U = 2.0**-24
ACTS = {None: 0, "silu": 1, "relu": 2}

# (S, K0, K1, N, E, act, X0 per member)
CASES = [
    (1, 5, 3, 1, 1, None, False),
    (65, 5, 3, 16, 3, "relu", False),
    (130, 33, 2, 70, 3, "silu", False),
    (65, 8, 0, 70, 1, "relu", True),
    (130, 8, 0, 16, 3, "silu", True),
    (1, 33, 2, 70, 3, "relu", False),
    (65, 33, 2, 1, 3, None, True),
    (130, 5, 3, 70, 1, None, False),
    (65, 8, 0, 1, 3, None, True),
    (1, 8, 0, 16, 1, "relu", True),
    (130, 33, 2, 16, 1, "relu", False),
    (65, 5, 3, 70, 3, "silu", True),
]


def _ext():
    from stoix_amd import ops

    return ops.ext(required=True)


def _draw(S, K0, K1, N, E, act, per_member, seed=0):
    """fp32 CPU operands of one layer. aux is the test's own saved H (ReLU:
    a quarter exact zeros, negatives kept) or Z (SiLU)."""
    g = torch.Generator().manual_seed(seed + S + 7 * K0 + 31 * N + 101 * E)
    r = lambda *s: torch.randn(*s, generator=g)
    aux = r(E, S, N)
    if act == "relu":
        aux[torch.rand(E, S, N, generator=g) < 0.25] = 0.0
    return dict(
        x0=r(E, S, K0) if per_member else r(S, K0), x1=r(S, K1) if K1 else None,
        W=[r(N, K0 + K1) for _ in range(E)], b=[r(N) for _ in range(E)], dH=r(E, S, N), aux=aux,
    )


def _x64(d, E):
    """[E, S, K] fp64 input with the pieces joined."""
    x0 = d["x0"].double()
    x0 = x0 if x0.dim() == 3 else x0.expand(E, *x0.shape)
    return x0 if d["x1"] is None else torch.cat([x0, d["x1"].double().expand(E, *d["x1"].shape)], -1)


def _dz64(d, act):
    dh, a = d["dH"].double(), d["aux"].double()
    if act == "relu":
        return dh * (a > 0)
    if act == "silu":
        s = torch.sigmoid(a)
        return dh * (s * (1 + a * (1 - s)))
    return dh


def _check(name, got, ref, bound):
    err = (got.detach().cpu().double() - ref).abs()
    worst = (err / bound.clamp_min(1e-300)).max().item() if (bound > 0).any() else 0.0
    print(f"{name}: max err {err.max().item():.3e}, worst err/bound {worst:.3f}")
    assert got.shape == ref.shape and (err <= bound).all(), name


def _dev(t):
    return torch.empty(0, device="cuda") if t is None else t.cuda()


@requires_gpu
@pytest.mark.parametrize("S,K0,K1,N,E,act,per_member", CASES)
def test_layer_kernels_match_fp64(S, K0, K1, N, E, act, per_member):
    ext = _ext()
    d = _draw(S, K0, K1, N, E, act, per_member)
    K = K0 + K1
    X, W, b = _x64(d, E), torch.stack(d["W"]).double(), torch.stack(d["b"]).double()
    x0, x1, Wd, bd = d["x0"].cuda(), _dev(d["x1"]), [w.cuda() for w in d["W"]], [v.cuda() for v in d["b"]]

    # forward
    Z64 = X @ W.transpose(1, 2) + b[:, None, :]
    bZ = (K + 3) * U * (X.abs() @ W.abs().transpose(1, 2) + b.abs()[:, None, :])
    H64 = torch.relu(Z64) if act == "relu" else (Z64 * torch.sigmoid(Z64) if act == "silu" else Z64)
    H = torch.empty(E, S, N, device="cuda")
    Z = torch.empty_like(H) if act == "silu" else torch.empty(0, device="cuda")
    assert ext.qens_linear_fwd(x0, x1, Wd, bd, Z, H, ACTS[act])
    if act == "silu":
        _check("Z", Z, Z64, bZ)
    _check("H", H, H64, bZ if act is None else 1.1 * bZ + 2.0**-21 * H64.abs())

    # backward: dZ formed in the kernels from dH and the test's own aux
    dZ = _dz64(d, act)
    dH, aux = d["dH"].cuda(), (_dev(None) if act is None else d["aux"].cuda())
    dX = torch.empty(E, S, K0, device="cuda")
    assert ext.qens_linear_dgrad(dH, aux, Wd, dX, 0, ACTS[act], False)
    _check("dX0", dX, dZ @ W[:, :, :K0], (N + 16) * U * (dZ.abs() @ W.abs()[:, :, :K0]))
    if K1:
        dA = torch.empty(S, K1, device="cuda")
        assert ext.qens_linear_dgrad(dH, aux, Wd, dA, K0, ACTS[act], True)
        _check("dX1 summed", dA, (dZ @ W[:, :, K0:]).sum(0),
               (E * N + 16) * U * (dZ.abs() @ W.abs()[:, :, K0:]).sum(0))
    dW = [torch.empty(N, K, device="cuda") for _ in range(E)]
    db = [torch.empty(N, device="cuda") for _ in range(E)]
    assert ext.qens_linear_wgrad(dH, aux, x0, x1, dW, db, ACTS[act])
    _check("dW", torch.stack(dW), dZ.transpose(1, 2) @ X, (S + 16) * U * (dZ.abs().transpose(1, 2) @ X.abs()))
    _check("db", torch.stack(db), dZ.sum(1), (S + 16) * U * dZ.abs().sum(1))


@requires_gpu
@pytest.mark.parametrize("N", [16, 70])  # 16-byte and 4-byte store paths
def test_outputs_stay_inside_their_rows_and_columns(N):
    ext = _ext()
    S, K0, E = 65, 8, 3
    d = _draw(S, K0, 0, N, E, "relu", True)
    Wd, bd = [w.cuda() for w in d["W"]], [v.cuda() for v in d["b"]]

    def framed(cols):
        big = torch.full((E, S + 2, cols + 8), float("nan"), device="cuda")
        return big, big[:, 1 : S + 1, 4 : cols + 4]

    big, H = framed(N)
    assert ext.qens_linear_fwd(d["x0"].cuda(), _dev(None), Wd, bd, _dev(None), H, ACTS["relu"])
    big2, dX = framed(K0)
    assert ext.qens_linear_dgrad(d["dH"].cuda(), d["aux"].cuda(), Wd, dX, 0, ACTS["relu"], False)
    for frame, inner in ((big, H), (big2, dX)):
        assert torch.isfinite(inner).all()
        inner.fill_(float("nan"))
        assert torch.isnan(frame).all()  # the margin was never written


@requires_gpu
def test_two_launches_give_the_same_bits():
    ext = _ext()
    S, K0, K1, N, E = 130, 33, 2, 70, 3
    d = _draw(S, K0, K1, N, E, "silu", False)
    x0, x1, Wd, bd = d["x0"].cuda(), d["x1"].cuda(), [w.cuda() for w in d["W"]], [v.cuda() for v in d["b"]]
    dH, aux = d["dH"].cuda(), d["aux"].cuda()
    runs = []
    for _ in range(2):
        H, Z, dA = torch.empty(E, S, N, device="cuda"), torch.empty(E, S, N, device="cuda"), torch.empty(S, K1, device="cuda")
        dW = [torch.empty(N, K0 + K1, device="cuda") for _ in range(E)]
        db = [torch.empty(N, device="cuda") for _ in range(E)]
        assert ext.qens_linear_fwd(x0, x1, Wd, bd, Z, H, 1)
        assert ext.qens_linear_dgrad(dH, aux, Wd, dA, K0, 1, True)
        assert ext.qens_linear_wgrad(dH, aux, x0, x1, dW, db, 1)
        runs.append([H, Z, dA, *dW, *db])
    assert all(torch.equal(a, b) for a, b in zip(*runs))


# ------------------------------------------------------------ module level

OBS, ACT_DIM, S_MOD = 11, 3, 65
# ReLU: a seed at which the fp64 reference on the CPU has no hidden
# pre-activation within 1e-4 of the kink (the nearest is 2.8e-4 away)
MODULE_SEED = {"relu": 41, "silu": 0}


def _ensemble(act, layer_norm=False):
    from stoix_amd.networks.base import FeedForwardCritic, MultiNetwork
    from stoix_amd.networks.heads import ScalarCriticHead
    from stoix_amd.networks.inputs import EmbeddingActionInput
    from stoix_amd.networks.torso import MLPTorso

    torch.manual_seed(MODULE_SEED[act])

    def member():  # as build_critic(..., obs_action_input=True) builds it
        torso = MLPTorso(OBS + ACT_DIM, [70, 70], activation=act, use_layer_norm=layer_norm)
        return FeedForwardCritic(torso, ScalarCriticHead(torso.output_dim), input_layer=EmbeddingActionInput())

    mn = MultiNetwork([member(), member()])
    for p in mn.parameters():
        if p.dim() == 1:
            nn.init.normal_(p, std=0.1)
    obs, action, w = torch.randn(S_MOD, OBS), torch.randn(S_MOD, ACT_DIM), torch.randn(2, S_MOD)
    return mn, obs, action, w


def _q_and_grads(mn, obs, action, w):
    action = action.detach().clone().requires_grad_(True)
    q = mn(obs, action)
    grads = torch.autograd.grad((q * w).sum(), [action, *mn.parameters()])
    return [q.detach(), *grads]


@requires_gpu
@pytest.mark.parametrize("act", ["relu", "silu"])
def test_module_matches_fp64_autograd_and_captures(act, monkeypatch):
    from stoix_amd.ops.qens import qens_route_to_kernel

    monkeypatch.setenv("STOIX_FUSED_QENS", "1")
    mn, obs, action, w = _ensemble(act)
    ref = _q_and_grads(copy.deepcopy(mn).double(), obs.double(), action.double(), w.double())
    chain = _q_and_grads(mn, obs, action, w)
    if act == "relu":  # a condition on the reference, not a tolerance
        mn64, x = copy.deepcopy(mn).double(), torch.cat([obs, action], -1).double()
        for net in mn64.networks:
            h = x
            for mod in net.torso.net:
                if isinstance(mod, nn.Linear):
                    assert mod(h).abs().min().item() >= 1e-4, "pre-activation too close to the ReLU kink"
                h = mod(h)

    dev = copy.deepcopy(mn).cuda()
    obs_d, act_d, w_d = obs.cuda(), action.cuda(), w.cuda()
    assert qens_route_to_kernel(dev, (obs_d, act_d))
    assert not qens_route_to_kernel(_ensemble(act, layer_norm=True)[0].cuda(), (obs_d, act_d))
    torch.cuda.set_sync_debug_mode("error")
    try:
        got = _q_and_grads(dev, obs_d, act_d, w_d)
    finally:
        torch.cuda.set_sync_debug_mode("default")
    assert got[0].shape == (2, S_MOD)
    names = ["q", "d action", *(n for n, _ in mn.named_parameters())]
    for name, k, r, c in zip(names, got, ref, chain):
        err, err_chain = (k.cpu().double() - r).abs().max().item(), (c.double() - r).abs().max().item()
        ulp = float(np.spacing(np.float32(r.abs().max().item())))
        print(f"{act} {name}: fused {err:.3e} chain {err_chain:.3e} ratio {err / max(err_chain, 1e-300):.3f}")
        assert k.shape == r.shape and err <= 2 * err_chain + ulp, name

    # captured once, replayed twice: the eager result's bits both times
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        _q_and_grads(dev, obs_d, act_d, w_d)
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out = _q_and_grads(dev, obs_d, act_d, w_d)
    for _ in range(2):
        for t in out:
            t.fill_(float("nan"))
        graph.replay()
        torch.cuda.synchronize()
        assert all(torch.equal(a, b) for a, b in zip(out, got))
