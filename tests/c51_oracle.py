"""Inputs and the fp64 oracle shared by the C51 loss tests (not a test file).

The oracle is the torch assembly the categorical losses are made of:
softmax -> greedy gather -> categorical_l2_project -> -(target * log_softmax),
run in fp64 on the CPU, with autograd for the gradient.
"""
import torch
import torch.nn.functional as F

from stoix_amd.ops import losses as L

VMIN, VMAX = -10.0, 10.0


def make_inputs(B, A, N, M, seed=0, dtype=torch.float32):
    """Random batch with the first five rows overwritten by the edge cases:
    identity, integral shift with clamped top atoms, all mass on the last /
    first atom, terminal point mass between two atoms."""
    g = torch.Generator().manual_seed(seed)
    z_tm1 = torch.linspace(VMIN, VMAX, M)
    z_t = torch.linspace(VMIN, VMAX, N)
    lt1 = (3 * torch.randn(B, A, M, generator=g)).to(dtype)
    lt = (3 * torch.randn(B, A, N, generator=g)).to(dtype)
    r = 4 * torch.randn(B, generator=g)
    d = 0.99 * torch.bernoulli(torch.full((B,), 0.8), generator=g)
    a = torch.randint(0, A, (B,), generator=g)
    sel = torch.randn(B, A, generator=g)
    dz = (VMAX - VMIN) / (M - 1)
    edge = [(0.0, 1.0), (3 * dz, 1.0), (100.0, 0.99), (-100.0, 0.99), (1.2345, 0.0)]
    for i, (ri, di) in enumerate(edge):
        r[i], d[i] = ri, di
    return dict(lt1=lt1, z_tm1=z_tm1, a=a, r=r, d=d, lt=lt, z_t=z_t, sel=sel)


def oracle(inp):
    """(ce [B], target [B, M], dlogits [B, A, M] for grad_ce = ones), fp64."""
    lt1 = inp["lt1"].double().detach().requires_grad_(True)
    lt = inp["lt"].double()
    B = lt1.shape[0]
    rows = torch.arange(B)
    best = inp["sel"].argmax(-1)
    p = F.softmax(lt, dim=-1)[rows, best]
    tz = inp["r"].double().unsqueeze(-1) + inp["d"].double().unsqueeze(-1) * inp["z_t"].double()
    target = L.categorical_l2_project(tz, p, inp["z_tm1"].double())
    ce = -(target * F.log_softmax(lt1[rows, inp["a"]], dim=-1)).sum(-1)
    (g,) = torch.autograd.grad(ce.sum(), lt1)
    return ce.detach(), target, g


def to_device(inp, device):
    return {k: v.to(device) for k, v in inp.items()}
