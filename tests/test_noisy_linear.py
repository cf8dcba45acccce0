"""CPU tests of the NoisyLinear routing (ops/noisy.py): the eligibility
decisions, and that with the knob on the CPU path of NoisyLinear / NoiseBank /
NoisyMLPTorso still returns the layer's formula, written out here."""
import pytest
import torch
import torch.nn.functional as F

from stoix_amd.networks.layers import NoiseBank, NoisyLinear
from stoix_amd.networks.torso import NoisyMLPTorso
from stoix_amd.ops.noisy import _noisy_kernel_eligible, noisy_route_to_kernel

BF16, FP32 = torch.bfloat16, torch.float32


@pytest.mark.parametrize(
    "knob,is_cuda,dtype,K,autocast,want",
    [
        ("1", True, FP32, 720, BF16, True),
        ("1", True, BF16, 8, BF16, True),
        ("1", True, FP32, 44, BF16, False),  # K % 8
        ("1", True, FP32, 4, BF16, False),
        ("1", True, torch.float16, 64, BF16, False),  # dtype
        ("1", True, FP32, 64, None, False),  # autocast off
        ("1", True, FP32, 64, torch.float16, False),
        ("1", False, FP32, 64, BF16, False),  # CPU
        ("0", True, FP32, 64, BF16, False),  # knob
    ],
)
def test_eligibility(monkeypatch, knob, is_cuda, dtype, K, autocast, want):
    monkeypatch.setenv("STOIX_FUSED_NOISY", knob)
    assert _noisy_kernel_eligible(is_cuda, dtype, K, autocast) is want


def formula(lin, x):
    w = lin.weight_mu + lin.weight_sigma * torch.outer(lin.eps_out, lin.eps_in)
    return F.linear(x, w, lin.bias_mu + lin.bias_sigma * lin.eps_out)


@pytest.mark.parametrize("act", [None, "silu", "relu"])
def test_cpu_layer_keeps_the_formula(monkeypatch, act):
    monkeypatch.setenv("STOIX_FUSED_NOISY", "1")
    torch.manual_seed(0)
    lin = NoisyLinear(24, 10)
    lin.resample_noise()
    x = torch.randn(5, 24)
    assert not noisy_route_to_kernel(x, lin)
    want = formula(lin, x)
    want = {None: lambda t: t, "silu": F.silu, "relu": F.relu}[act](want)
    assert torch.equal(lin(x, act=act), want)
    with torch.autocast("cpu", torch.bfloat16):  # CPU autocast does not route either
        assert lin(x, act=act).shape == want.shape and lin._mat is None


def test_cpu_bank_and_torso_unchanged(monkeypatch):
    monkeypatch.setenv("STOIX_FUSED_NOISY", "1")
    torch.manual_seed(1)
    torso = NoisyMLPTorso(24, (16, 8), activation="silu")
    bank = NoiseBank(torso)
    g = torch.Generator().manual_seed(5)
    bank.resample(g)
    n = torch.empty(bank.flat.numel()).normal_(generator=torch.Generator().manual_seed(5))
    assert torch.equal(bank.flat, n.sign() * n.abs().sqrt())
    assert all(m._mat is not None for m in bank.layers)  # CPU: materialised as before
    x = torch.randn(3, 24)
    l1, l2 = bank.layers
    assert torch.equal(torso(x), F.silu(formula(l2, F.silu(formula(l1, x)))))
