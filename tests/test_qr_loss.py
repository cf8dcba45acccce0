"""Per-row QR-DQN loss (ops/losses.py::quantile_q_learning_rows) on the CPU:
its mean is quantile_q_learning bit for bit, it matches the fp64 oracle, and
the STOIX_FUSED_QR knob changes nothing for CPU tensors."""
import pytest
import torch

from qr_oracle import make_inputs, oracle
from stoix_amd.ops import losses as L

KEYS = ("src", "tau", "a", "r", "d", "sel", "tgt")


@pytest.mark.parametrize("k", [1.0, 0.5, 0.0])
def test_rows_mean_is_quantile_q_learning_on_cpu_whatever_the_knob(monkeypatch, k):
    inp = make_inputs(11, 2, 130, 33)
    args = tuple(inp[n] for n in KEYS)
    out = {}
    for knob in ("1", "0"):
        monkeypatch.setenv("STOIX_FUSED_QR", knob)
        assert L.qr_fused_enabled() == (knob == "1")
        rows = L.quantile_q_learning_rows(*args, k)
        assert rows.shape == (11,)
        assert torch.equal(rows.mean(), L.quantile_q_learning(*args, k))
        out[knob] = rows
    assert torch.equal(out["1"], out["0"])
    loss_ref, _ = oracle(inp, k)
    torch.testing.assert_close(out["1"].double(), loss_ref, rtol=1e-4, atol=1e-4)
