"""K13 training scan on the GPU: ``rnn_scan_train_fwd`` / ``rnn_scan_bwd``
(ops/csrc/rnn.hip) behind ops/rnn.py ``_RnnScan`` and the grad-enabled
dispatch of ``ScannedRNN``.

Gradient accuracy is measured against two references, never against the
code under test: ``ref64`` (fp64 CPU autograd through ``_hoisted_scan``) and
``emul`` (an fp32 torch scan that rounds where the kernels round: W_hh to
bf16, the h fed to the recurrent linear to bf16 with a straight-through
gradient, the gradient of the recurrent pre-activation to bf16). The kernels
and ``emul`` differ only in summation order and ``__expf``, so their errors
against ``ref64`` are two draws of the same statistic: the bound is
``err(kernel) <= 2 * err(emul)`` per input.
"""
import functools
import os
import subprocess
import sys

import pytest
import torch
import torch.nn.functional as F

pytestmark = [
    pytest.mark.gpu,
    pytest.mark.skipif(not torch.cuda.is_available(), reason="no GPU"),
]

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
D = 20
NAMES = ["x", "h0", "c0", "W_ih", "b_ih", "W_hh", "b_hh"]
KINDS = [("gru", 128), ("gru", 256), ("lstm", 128), ("lstm", 256)]
# two full 16-row tiles plus a 5-row tail; and the single-step single-tile case
SHAPES = [(7, 37), (1, 16)]


class _RoundSTE(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x):
        return x.to(torch.bfloat16).to(x.dtype)

    @staticmethod
    def backward(ctx, g):
        return g


class _RoundGrad(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x):
        return x.view_as(x)

    @staticmethod
    def backward(ctx, g):
        return g.to(torch.bfloat16).to(g.dtype)


def _emul_scan(kind, x, resets, h0, c0, w_ih, b_ih, w_hh, b_hh):
    T, B = x.shape[:2]
    xp = F.linear(x.reshape(T * B, -1), w_ih, b_ih).reshape(T, B, -1)
    w = _RoundSTE.apply(w_hh)
    h, c = h0, c0
    outs = []
    for t in range(T):
        keep = (~resets[t]).to(x.dtype).unsqueeze(-1)
        h = h * keep
        hg = _RoundGrad.apply(F.linear(_RoundSTE.apply(h), w)) + b_hh
        if kind == "gru":
            xr, xz, xn = xp[t].chunk(3, -1)
            hr, hz, hn = hg.chunk(3, -1)
            r = torch.sigmoid(xr + hr)
            z = torch.sigmoid(xz + hz)
            n = torch.tanh(xn + r * hn)
            h = (1 - z) * n + z * h
        else:
            c = c * keep
            i, f, g, o = (xp[t] + hg).chunk(4, -1)
            c = torch.sigmoid(f) * c + torch.sigmoid(i) * torch.tanh(g)
            h = torch.sigmoid(o) * torch.tanh(c)
        outs.append(h)
    return torch.stack(outs), h, c


def _make_rnn(kind, H):
    from stoix_amd.networks.base import ScannedRNN

    torch.manual_seed(1234)
    return ScannedRNN(D, H, cell_type=kind)


def _params(rnn):
    cell, _ = rnn._single_cell()
    return [cell.weight_ih, cell.bias_ih, cell.weight_hh, cell.bias_hh]


def _loss(kind, Hout, hT, cT, w):
    loss = (Hout * w[0]).sum() + (hT * w[1]).sum()
    if kind == "lstm":
        loss = loss + (cT * w[2]).sum()
    return loss


@functools.lru_cache(maxsize=None)
def _case(kind, H, T, B):
    """Inputs plus the two CPU references, computed once per shape."""
    g = torch.Generator().manual_seed(100 * T + B + H)
    x = torch.randn(T, B, D, generator=g)
    resets = torch.rand(T, B, generator=g) < 0.15
    resets[0, 0] = True  # forced: reset at t=0
    resets[:, 1] = True  # reset at every step
    resets[:, 2] = False  # never reset
    h0 = 0.5 * torch.randn(B, H, generator=g)
    c0 = 0.5 * torch.randn(B, H, generator=g)
    w = tuple(torch.randn(s, generator=g) for s in ((T, B, H), (B, H), (B, H)))

    # ref64: fp64 CPU autograd through _hoisted_scan
    rnn64 = _make_rnn(kind, H).double()
    cell64, _ = rnn64._single_cell()
    ins = [t.double().requires_grad_() for t in (x, h0, c0)]
    state = [(ins[1], ins[2])] if kind == "lstm" else [ins[1]]
    Hout, st = rnn64._hoisted_scan(ins[0], resets, state, cell64, kind)
    hT, cT = st[0] if kind == "lstm" else (st[0], None)
    g64 = torch.autograd.grad(
        _loss(kind, Hout, hT, cT, [t.double() for t in w]), ins + _params(rnn64), allow_unused=True
    )

    # emul: fp32 CPU scan with the kernels' rounding points
    rnn32 = _make_rnn(kind, H)
    ins = [t.clone().requires_grad_() for t in (x, h0, c0)]
    Hout, hT, cT = _emul_scan(kind, ins[0], resets, ins[1], ins[2], *_params(rnn32))
    gem = torch.autograd.grad(_loss(kind, Hout, hT, cT, w), ins + _params(rnn32), allow_unused=True)
    return dict(x=x, resets=resets, h0=h0, c0=c0, w=w, g64=g64, gemul=gem)


def _gpu_forward(kind, rnn, case, grad):
    x = case["x"].cuda().requires_grad_(grad)
    h0 = case["h0"].cuda().requires_grad_(grad)
    c0 = case["c0"].cuda().requires_grad_(grad)
    state = [(h0, c0)] if kind == "lstm" else [h0]
    with torch.set_grad_enabled(grad):
        Hout, st = rnn(x, case["resets"].cuda(), state)
    hT, cT = st[0] if kind == "lstm" else (st[0], None)
    return (x, h0, c0), (Hout, hT, cT)


@pytest.mark.parametrize("T,B", SHAPES)
@pytest.mark.parametrize("kind,H", KINDS)
def test_train_forward_bit_equal_to_no_grad(kind, H, T, B):
    """With gradients on, the module runs the training kernel and returns
    exactly what the no-grad kernel returns."""
    case = _case(kind, H, T, B)
    rnn = _make_rnn(kind, H).cuda()
    _, out_g = _gpu_forward(kind, rnn, case, grad=True)
    _, out_n = _gpu_forward(kind, rnn, case, grad=False)
    assert type(out_g[0].grad_fn).__name__ == "_RnnScanBackward"
    for name, a, b in zip(("Hout", "hT", "cT"), out_g, out_n):
        if a is None:
            assert kind == "gru" and b is None
            continue
        assert torch.isfinite(a).all(), name
        assert torch.equal(a.detach(), b), name


def _err(g, ref):
    return float((g.double() - ref).abs().max()) / float(ref.abs().max())


@pytest.mark.parametrize("T,B", SHAPES)
@pytest.mark.parametrize("kind,H", KINDS)
def test_gradients_within_twice_the_emulation_error(kind, H, T, B):
    case = _case(kind, H, T, B)
    rnn = _make_rnn(kind, H).cuda()
    ins, (Hout, hT, cT) = _gpu_forward(kind, rnn, case, grad=True)
    loss = _loss(kind, Hout, hT, cT, [t.cuda() for t in case["w"]])
    gk = torch.autograd.grad(loss, list(ins) + _params(rnn), allow_unused=True)
    failed = []
    for name, k, e, r in zip(NAMES, gk, case["gemul"], case["g64"]):
        if name == "c0" and kind == "gru":
            assert k is None and r is None
            continue
        ek, ee = _err(k.cpu(), r), _err(e, r)
        print(f"{kind} H={H} T={T} B={B} {name:5s} err(kernel)={ek:.3e} err(emul)={ee:.3e} ratio={ek / ee:.3f}")
        assert ee > 0.0, name
        if not ek <= 2.0 * ee:
            failed.append((name, ek, ee))
    assert not failed, failed
    # a row reset at t=0 never sees its initial state
    assert torch.equal(gk[1][0], torch.zeros_like(gk[1][0]))
    if kind == "lstm":
        assert torch.equal(gk[2][0], torch.zeros_like(gk[2][0]))


def _scan_inputs(kind, H, T, B, seed):
    """Leaf inputs of the autograd node itself (xp, not x), on the GPU."""
    g = torch.Generator().manual_seed(seed)
    G = 3 if kind == "gru" else 4
    k = H**-0.5
    xp = torch.randn(T, B, G * H, generator=g)
    whh = (torch.rand(G * H, H, generator=g) * 2 - 1) * k
    bhh = (torch.rand(G * H, generator=g) * 2 - 1) * k
    h0 = 0.5 * torch.randn(B, H, generator=g)
    c0 = 0.5 * torch.randn(B, H, generator=g)
    resets = torch.rand(T, B, generator=g) < 0.15
    resets[0, 0] = True
    resets[:, 1] = True
    resets[:, 2] = False
    return [t.cuda() for t in (xp, whh, bhh, h0, c0)], resets.cuda()


def _scan_grads(kind, tensors, resets, loss_fn):
    from stoix_amd.ops.rnn import rnn_scan

    xp, whh, bhh, h0, c0 = [t.detach().clone().requires_grad_() for t in tensors]
    out = rnn_scan(xp, whh, bhh, resets, h0, c0 if kind == "lstm" else None, kind)
    leaves = [xp, h0, whh, bhh] + ([c0] if kind == "lstm" else [])
    grads = torch.autograd.grad(loss_fn(out), leaves)
    return out, dict(zip(["dXp", "dh0", "dWhh", "dbhh", "dc0"], grads))


@pytest.mark.parametrize("kind,H", KINDS)
def test_strided_dhout_and_missing_dhT(kind, H):
    """The stride-0 gradient of Hout.sum() with no gradient at all through
    hT/cT equals the materialised ones/zeros form."""
    T, B = 7, 37
    tensors, resets = _scan_inputs(kind, H, T, B, seed=7)
    _, lazy = _scan_grads(kind, tensors, resets, lambda out: out[0].sum())

    def dense(out):
        loss = (out[0] * torch.ones_like(out[0])).sum()
        for o in out[1:]:
            loss = loss + (o * torch.zeros_like(o)).sum()
        return loss

    _, full = _scan_grads(kind, tensors, resets, dense)
    for name in lazy:
        assert torch.isfinite(lazy[name]).all(), name
        if name in ("dWhh", "dbhh"):
            # library GEMM / reduction over identical operands
            torch.testing.assert_close(lazy[name], full[name], rtol=1e-6, atol=1e-6)
        else:
            assert torch.equal(lazy[name], full[name]), name


@pytest.mark.parametrize("kind,H", KINDS)
def test_deterministic_and_graph_capturable(kind, H):
    """Two eager runs are bit-equal, and forward + backward captured once in
    a graph on one stream replays bit-equal to eager on refreshed inputs."""
    from stoix_amd.ops.rnn import rnn_scan

    T, B = 7, 37
    sets = [_scan_inputs(kind, H, T, B, seed=s) for s in (11, 12)]
    g = torch.Generator().manual_seed(5)
    w = [torch.randn(s, generator=g).cuda() for s in ((T, B, H), (B, H), (B, H))]
    loss_fn = lambda out: sum((o * wi).sum() for o, wi in zip(out, w))
    names = ["dXp", "dh0"] + (["dc0"] if kind == "lstm" else [])

    eager = []
    for tensors, resets in sets:
        out_a, ga = _scan_grads(kind, tensors, resets, loss_fn)
        out_b, gb = _scan_grads(kind, tensors, resets, loss_fn)
        for name in names:
            assert torch.equal(ga[name], gb[name]), name
        assert torch.equal(out_a[0], out_b[0])
        eager.append((out_a[0].detach().clone(), {n: ga[n].clone() for n in names}))

    static = [t.clone().requires_grad_() for t in sets[0][0]]
    static_resets = sets[0][1].clone()
    xp, whh, bhh, h0, c0 = static
    leaves = [xp, h0] + ([c0] if kind == "lstm" else [])

    def step():
        out = rnn_scan(xp, whh, bhh, static_resets, h0, c0 if kind == "lstm" else None, kind)
        return out[0], torch.autograd.grad(loss_fn(out), leaves)

    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        step()
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        static_out, static_grads = step()

    for idx in (1, 0):  # refreshed inputs first, then back to the captured ones
        tensors, resets = sets[idx]
        with torch.no_grad():
            for dst, src in zip(static, tensors):
                dst.copy_(src)
            static_resets.copy_(resets)
        graph.replay()
        torch.cuda.synchronize()
        out_e, grads_e = eager[idx]
        assert torch.equal(static_out.detach(), out_e)
        for name, got in zip(names, static_grads):
            assert torch.equal(got, grads_e[name]), (idx, name)


_CHILD = """
import torch
from stoix_amd.networks.base import ScannedRNN
torch.manual_seed(0)
for kind in ("gru", "lstm"):
    rnn = ScannedRNN(20, 128, cell_type=kind).cuda()
    cell, _ = rnn._single_cell()
    x = torch.randn(5, 19, 20, device="cuda", requires_grad=True)
    resets = torch.rand(5, 19, device="cuda") < 0.2
    st = rnn.initial_state(19, "cuda")
    out, s1 = rnn(x, resets, list(st))
    ref, s2 = rnn._hoisted_scan(x, resets, list(st), cell, kind)
    assert type(out.grad_fn).__name__ != "_RnnScanBackward", out.grad_fn
    assert torch.equal(out, ref)
    a, b = (s1[0], s2[0]) if kind == "gru" else (torch.cat(s1[0]), torch.cat(s2[0]))
    assert torch.equal(a, b)
print("FALLBACK_OK")
"""


def test_fallback_switch_restores_hoisted_scan():
    """STOIX_FUSED_RNN=0, set in a fresh process, puts the grad-enabled scan
    back on ``_hoisted_scan``."""
    env = dict(os.environ, STOIX_FUSED_RNN="0")
    env["PYTHONPATH"] = REPO + os.pathsep + env.get("PYTHONPATH", "")
    out = subprocess.run(
        [sys.executable, "-c", _CHILD], capture_output=True, text=True, timeout=300, cwd=REPO, env=env
    )
    assert out.returncode == 0, f"{out.stdout}\n{out.stderr}"
    assert "FALLBACK_OK" in out.stdout
