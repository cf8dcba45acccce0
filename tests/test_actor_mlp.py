"""CPU tests of the fused-actor routing (ops/actor_mlp.py): what the kernels
accept, and that a CPU actor keeps its module chain whatever the knob says."""
import pytest
import torch

from stoix_amd.networks.base import FeedForwardActor
from stoix_amd.networks.heads import BetaDistributionHead, NormalAffineTanhDistributionHead
from stoix_amd.networks.torso import CNNTorso, MLPTorso
from stoix_amd.ops.actor_mlp import actor_layers, actor_route_to_kernel

OBS, ACT_DIM = 27, 5


def _actor(torso=None, head=None):
    torso = torso or MLPTorso(OBS, [256, 256], activation="silu")  # network/mlp_continuous
    head = head or NormalAffineTanhDistributionHead(torso.output_dim, ACT_DIM, -1.0, 1.0)
    return FeedForwardActor(torso, head)


@pytest.mark.parametrize("knob", ["0", "1"])
def test_cpu_actor_keeps_the_module_chain(knob, monkeypatch):
    monkeypatch.setenv("STOIX_FUSED_ACTOR", knob)
    torch.manual_seed(0)
    actor, obs = _actor(), torch.randn(9, OBS)
    assert not actor_route_to_kernel(actor, obs)
    dist, want = actor(obs), actor.action_head(actor.torso(obs))
    assert torch.equal(dist.base.loc, want.base.loc) and torch.equal(dist.base.scale, want.base.scale)


def test_actor_layers_accepts_the_mlp_continuous_actor():
    layers = actor_layers(_actor())
    assert [lin.out_features for lin in layers.hidden] == [256, 256] and layers.act == "silu"
    assert layers.head.loc.out_features == ACT_DIM


@pytest.mark.parametrize("actor", [
    _actor(MLPTorso(OBS, [256, 256], use_layer_norm=True)),
    _actor(CNNTorso((1, 36, 36), mlp_sizes=(64,))),
    _actor(head=BetaDistributionHead(256, ACT_DIM, -1.0, 1.0)),
], ids=["layer_norm", "cnn_torso", "beta_head"])
def test_actor_layers_rejects(actor):
    assert actor_layers(actor) is None
