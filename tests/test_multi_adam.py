"""OptimTail on CPU tensors: with either value of STOIX_FUSED_OPTIM it is the
three torch calls it replaces, bit for bit, and an inactive chain (TD3's
delayed actor) is left untouched."""
import copy

import pytest
import torch
import torch.nn as nn

from stoix_amd.ops.optim import OptimChain, OptimTail
from stoix_amd.parallel.dist import polyak_update


def _nets(seed):
    torch.manual_seed(seed)
    net = nn.Sequential(nn.Linear(5, 7), nn.Tanh(), nn.Linear(7, 3))
    net(torch.randn(11, 5)).square().sum().backward()
    tgt = copy.deepcopy(net).requires_grad_(False)
    with torch.no_grad():
        for p in tgt.parameters():
            p.add_(0.1)
    return net, tgt, torch.optim.Adam(net.parameters(), lr=1e-2)


@pytest.mark.parametrize("knob", ["0", "1"])
@pytest.mark.parametrize("active", [None, (True, False)])
def test_cpu_step_is_the_torch_calls(monkeypatch, knob, active):
    monkeypatch.setenv("STOIX_FUSED_OPTIM", knob)
    (q, q_t, q_opt), (a, a_t, a_opt) = _nets(0), _nets(1)
    tail = OptimTail([OptimChain(q_opt, q.parameters(), 0.5, q_t.parameters(), 0.25),
                      OptimChain(a_opt, a.parameters(), None, a_t.parameters(), 0.25)])
    (q2, q2_t, q2_opt), (a2, a2_t, a2_opt) = _nets(0), _nets(1)
    a_before = copy.deepcopy((a.state_dict(), a_t.state_dict()))
    for _ in range(2):
        assert tail.step(active) is False
        nn.utils.clip_grad_norm_(q2.parameters(), 0.5)
        q2_opt.step()
        if active is None:
            a2_opt.step()
        with torch.no_grad():
            polyak_update(q2.parameters(), q2_t.parameters(), 0.25)
            if active is None:
                polyak_update(a2.parameters(), a2_t.parameters(), 0.25)
    for got, want in ((q, q2), (q_t, q2_t), (a, a2), (a_t, a2_t)):
        assert all(torch.equal(x, y) for x, y in zip(got.parameters(), want.parameters()))
    if active is not None:  # the delayed chain: nothing moved, no state made
        for sd, before in zip((a.state_dict(), a_t.state_dict()), a_before):
            assert all(torch.equal(sd[k], before[k]) for k in sd)
        assert len(a_opt.state) == 0
