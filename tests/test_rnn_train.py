"""K13 training scan, CPU side: the closed-form backward of ops/rnn.py
``_RnnScan`` checked in fp64 against finite differences and against autograd
through ``ScannedRNN._hoisted_scan``."""
import pytest
import torch

from stoix_amd.networks.base import ScannedRNN
from stoix_amd.ops.rnn import _RnnScan

H, T, B, D = 8, 5, 3, 6
NAMES = ["x", "h0", "c0", "W_ih", "b_ih", "W_hh", "b_hh"]


def _resets():
    """Row 0 is reset at t=0 (and once more), row 1 at every step, row 2
    never."""
    rs = torch.zeros(T, B, dtype=torch.bool)
    rs[0, 0] = True
    rs[3, 0] = True
    rs[:, 1] = True
    return rs


def _case(kind, seed=0):
    g = torch.Generator().manual_seed(seed)
    G = 3 if kind == "gru" else 4
    rnn = ScannedRNN(D, H, cell_type=kind).double()
    cell, k = rnn._single_cell()
    assert k == kind
    with torch.no_grad():
        for p in cell.parameters():
            p.copy_(torch.randn(p.shape, generator=g, dtype=torch.float64) * 0.4)
    x = torch.randn(T, B, D, generator=g, dtype=torch.float64)
    h0 = 0.5 * torch.randn(B, H, generator=g, dtype=torch.float64)
    c0 = 0.5 * torch.randn(B, H, generator=g, dtype=torch.float64)
    w = [
        torch.randn(T, B, H, generator=g, dtype=torch.float64),
        torch.randn(B, H, generator=g, dtype=torch.float64),
        torch.randn(B, H, generator=g, dtype=torch.float64),
    ]
    assert cell.weight_hh.shape == (G * H, H)
    return rnn, cell, x, h0, c0, w


def _loss(kind, Hout, hT, cT, w):
    loss = (Hout * w[0]).sum() + (hT * w[1]).sum()
    if kind == "lstm":
        loss = loss + (cT * w[2]).sum()
    return loss


def _grads_fused(kind, cell, x, h0, c0, w, resets):
    ins = [t.detach().clone().requires_grad_() for t in (x, h0, c0)]
    ps = [cell.weight_ih, cell.bias_ih, cell.weight_hh, cell.bias_hh]
    xp = torch.nn.functional.linear(ins[0].reshape(T * B, -1), ps[0], ps[1]).reshape(T, B, -1)
    out = _RnnScan.apply(xp, ps[2], ps[3], resets, ins[1], ins[2] if kind == "lstm" else None, kind)
    loss = _loss(kind, out[0], out[1], out[2] if kind == "lstm" else None, w)
    return torch.autograd.grad(loss, ins + ps, allow_unused=True)


def _grads_hoisted(kind, rnn, cell, x, h0, c0, w, resets):
    ins = [t.detach().clone().requires_grad_() for t in (x, h0, c0)]
    ps = [cell.weight_ih, cell.bias_ih, cell.weight_hh, cell.bias_hh]
    state = [(ins[1], ins[2])] if kind == "lstm" else [ins[1]]
    Hout, st = rnn._hoisted_scan(ins[0], resets, state, cell, kind)
    hT, cT = st[0] if kind == "lstm" else (st[0], None)
    loss = _loss(kind, Hout, hT, cT, w)
    return torch.autograd.grad(loss, ins + ps, allow_unused=True)


@pytest.mark.parametrize("kind", ["gru", "lstm"])
def test_rnn_scan_gradcheck_fp64(kind):
    """Finite differences through every differentiable input, with gradients
    arriving through Hout, hT and cT."""
    _, cell, x, h0, c0, w = _case(kind)
    resets = _resets()
    xp = torch.nn.functional.linear(x.reshape(T * B, -1), cell.weight_ih, cell.bias_ih)
    xp = xp.reshape(T, B, -1).detach().requires_grad_()
    whh = cell.weight_hh.detach().clone().requires_grad_()
    bhh = cell.bias_hh.detach().clone().requires_grad_()
    h0 = h0.clone().requires_grad_()
    c0 = c0.clone().requires_grad_()

    if kind == "lstm":
        fn = lambda xp_, whh_, bhh_, h0_, c0_: _RnnScan.apply(xp_, whh_, bhh_, resets, h0_, c0_, kind)
        args = (xp, whh, bhh, h0, c0)
    else:
        fn = lambda xp_, whh_, bhh_, h0_: _RnnScan.apply(xp_, whh_, bhh_, resets, h0_, None, kind)
        args = (xp, whh, bhh, h0)
    assert len(fn(*args)) == (3 if kind == "lstm" else 2)
    assert torch.autograd.gradcheck(fn, args, eps=1e-6, atol=1e-6, rtol=1e-5)


@pytest.mark.parametrize("kind", ["gru", "lstm"])
def test_rnn_scan_matches_hoisted_autograd_fp64(kind):
    """Forward and every input gradient equal autograd through
    ``_hoisted_scan`` in fp64 at rtol = atol = 1e-10."""
    rnn, cell, x, h0, c0, w = _case(kind, seed=1)
    resets = _resets()
    got = _grads_fused(kind, cell, x, h0, c0, w, resets)
    ref = _grads_hoisted(kind, rnn, cell, x, h0, c0, w, resets)
    for name, a, b in zip(NAMES, got, ref):
        if name == "c0" and kind == "gru":
            assert a is None and b is None
            continue
        assert a is not None and b is not None, name
        torch.testing.assert_close(a, b, rtol=1e-10, atol=1e-10, msg=lambda m, n=name: f"{n}: {m}")

    with torch.no_grad():
        xp = torch.nn.functional.linear(x.reshape(T * B, -1), cell.weight_ih, cell.bias_ih).reshape(T, B, -1)
        out = _RnnScan.apply(xp, cell.weight_hh, cell.bias_hh, resets, h0, c0 if kind == "lstm" else None, kind)
        state = [(h0, c0)] if kind == "lstm" else [h0]
        Hout, st = rnn._hoisted_scan(x, resets, state, cell, kind)
    torch.testing.assert_close(out[0], Hout, rtol=1e-10, atol=1e-10)
    torch.testing.assert_close(out[1], st[0][0] if kind == "lstm" else st[0], rtol=1e-10, atol=1e-10)
    if kind == "lstm":
        torch.testing.assert_close(out[2], st[0][1], rtol=1e-10, atol=1e-10)


@pytest.mark.parametrize("kind", ["gru", "lstm"])
def test_rnn_scan_reset_row_has_zero_initial_state_grad(kind):
    """A row reset at t=0 never sees h0/c0: their gradients are exactly 0
    there and non-zero for the row that is never reset."""
    _, cell, x, h0, c0, w = _case(kind, seed=2)
    got = dict(zip(NAMES, _grads_fused(kind, cell, x, h0, c0, w, _resets())))
    for name in ("h0", "c0") if kind == "lstm" else ("h0",):
        g = got[name]
        assert torch.equal(g[0], torch.zeros_like(g[0])), name
        assert torch.equal(g[1], torch.zeros_like(g[1])), name
        assert float(g[2].abs().max()) > 0.0, name


@pytest.mark.parametrize("kind", ["gru", "lstm"])
def test_rnn_scan_accepts_missing_output_grads(kind):
    """A loss that uses only Hout (dhT, dcT are None) or only hT (dHout is
    None) gives the gradients of the same loss with explicit zero weights."""
    _, cell, x, h0, c0, w = _case(kind, seed=3)
    resets = _resets()
    zero = [torch.zeros_like(t) for t in w]
    for keep_idx in (0, 1):
        ins = [t.detach().clone().requires_grad_() for t in (x, h0, c0)]
        xp = torch.nn.functional.linear(ins[0].reshape(T * B, -1), cell.weight_ih, cell.bias_ih).reshape(T, B, -1)
        out = _RnnScan.apply(xp, cell.weight_hh, cell.bias_hh, resets, ins[1], ins[2] if kind == "lstm" else None, kind)
        loss = (out[keep_idx] * w[keep_idx]).sum()
        got = torch.autograd.grad(loss, ins[:2] + [cell.weight_hh, cell.bias_hh])
        ww = list(zero)
        ww[keep_idx] = w[keep_idx]
        ref = _grads_fused(kind, cell, x, h0, c0, ww, resets)
        for a, b in zip(got, [ref[0], ref[1], ref[5], ref[6]]):
            torch.testing.assert_close(a, b, rtol=1e-12, atol=1e-12)
