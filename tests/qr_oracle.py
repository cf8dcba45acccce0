"""Inputs and the fp64 oracle shared by the QR loss tests (not a test file).

The oracle forms the target samples r + d * tgt[:, :, best] in fp32 (two
torch ops on the CPU, so not fused), then runs the torch composition of
quantile_regression_loss in fp64, with autograd for the gradient. fl(t - th)
has the sign of t - th, so an fp32 kernel takes the same indicator [dl < 0]
on every pair.
"""
import torch


def make_inputs(B, A, N, M, seed=0, dtype=torch.float32):
    """Random batch; the selector [B, M, A] carries a per-row permutation of
    0.5 * arange(A) on the action axis, so its action means are about 0.25
    apart or more and no summation order flips the argmax. Edge rows: 0 an
    exact tie dl = 0 with every target sample, 1 and 2 all pairs on the
    linear branch, 3 (A > 1) an exact argmax tie between actions 0 and 1."""
    g = torch.Generator().manual_seed(seed)
    src = (2 * torch.randn(B, N, A, generator=g)).to(dtype)
    tgt = (2 * torch.randn(B, M, A, generator=g)).to(dtype)
    tau = (torch.arange(N, dtype=torch.float32) + 0.5) / N
    sel = torch.randn(B, M, A, generator=g)
    for b in range(B):
        sel[b] += 0.5 * torch.randperm(A, generator=g).float()
    r = 2 * torch.randn(B, generator=g)
    d = 0.99 * torch.bernoulli(torch.full((B,), 0.8), generator=g)
    a = torch.randint(0, A, (B,), generator=g)
    d[:3] = 0.0
    r[0], r[1], r[2] = float(src[0, N // 2, a[0]]), 100.0, -100.0
    if A > 1:
        sel[3, :, 1] = sel[3, :, 0]
        sel[3, :, 2:] = sel[3, :, :1] - 10.0
    return dict(src=src, tau=tau, a=a, r=r, d=d, sel=sel.to(dtype), tgt=tgt)


def oracle(inp, k):
    """(loss [B], dsrc [B, N, A] for a gradient of ones), fp64."""
    src = inp["src"].double().requires_grad_(True)
    rows = torch.arange(src.shape[0])
    best = inp["sel"].double().mean(1).argmax(-1)
    t = inp["r"].unsqueeze(-1) + inp["d"].unsqueeze(-1) * inp["tgt"].float()[rows, :, best]
    delta = t.double().unsqueeze(1) - src[rows, :, inp["a"]].unsqueeze(2)  # [B, N, M]
    weight = (inp["tau"].double().view(1, -1, 1) - (delta < 0).double()).abs()
    if k > 0:
        ad = delta.abs()
        rho = torch.where(ad <= k, 0.5 * delta**2, k * (ad - 0.5 * k)) / k
    else:
        rho = delta.abs()
    loss = (weight * rho).mean(2).sum(1)
    (g,) = torch.autograd.grad(loss.sum(), src)
    return loss.detach(), g


def to_device(inp, device):
    return {k: v.to(device) for k, v in inp.items()}
