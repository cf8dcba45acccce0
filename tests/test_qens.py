"""CPU tests of the Q-ensemble routing (ops/qens.py): the knob changes nothing
off the GPU, and the eligibility checks reject what the kernels do not take."""
import pytest
import torch

from stoix_amd.networks.base import FeedForwardCritic, MultiNetwork
from stoix_amd.networks.heads import ScalarCriticHead
from stoix_amd.networks.inputs import EmbeddingActionInput, EmbeddingActionOnehotInput
from stoix_amd.networks.torso import MLPTorso
from stoix_amd.ops.qens import _qens_tensor_eligible, qens_layers, qens_route_to_kernel


def _ensemble(members, input_layer=EmbeddingActionInput, in_dim=14):
    def member():
        torso = MLPTorso(in_dim, [24, 24], activation="relu")
        return FeedForwardCritic(torso, ScalarCriticHead(24), input_layer=input_layer())

    return MultiNetwork([member() for _ in range(members)])


def test_cpu_ensemble_is_bit_identical_with_either_knob_value(monkeypatch):
    torch.manual_seed(0)
    mn, obs, action = _ensemble(2), torch.randn(9, 11), torch.randn(9, 3, requires_grad=True)
    runs = []
    for knob in ("0", "1"):
        monkeypatch.setenv("STOIX_FUSED_QENS", knob)
        assert not qens_route_to_kernel(mn, (obs, action))
        q = mn(obs, action)
        runs.append([q.detach(), *torch.autograd.grad(q.square().sum(), [action, *mn.parameters()])])
    assert runs[0][0].shape == (2, 9) and all(torch.equal(a, b) for a, b in zip(*runs))


@pytest.mark.parametrize("members,expected", [(1, 3), (4, 3), (5, None)])
def test_member_count_limits(members, expected):
    layers = qens_layers(_ensemble(members))
    assert (layers and len(layers)) == expected


def test_onehot_members_and_bf16_inputs_are_rejected():
    onehot = _ensemble(2, input_layer=lambda: EmbeddingActionOnehotInput(3))
    assert qens_layers(onehot) is None
    assert _qens_tensor_eligible(True, torch.float32, 2, 10)
    assert not _qens_tensor_eligible(True, torch.bfloat16, 2, 10)
    assert not _qens_tensor_eligible(False, torch.float32, 2, 10)
