"""C51 categorical TD cross-entropy (ops/losses.py::c51_td_cross_entropy) on
the CPU: the closed-form backward and the fixed hi = min(lo + 1, M - 1)
projection against the fp64 torch assembly with autograd."""
import pytest
import torch

from c51_oracle import make_inputs, oracle
from stoix_amd.ops import losses as L

SHAPES = [(67, 3, 51, 51), (9, 1, 5, 5), (13, 4, 130, 130), (11, 2, 51, 33)]
TOL = dict(rtol=1e-9, atol=1e-12)


def _fp64(inp):
    out = {k: (v.double() if v.is_floating_point() else v) for k, v in inp.items()}
    out["lt1"].requires_grad_(True)
    return out


@pytest.mark.parametrize("shape", SHAPES)
def test_c51_td_cross_entropy_fp64_matches_autograd_assembly(shape):
    inp = make_inputs(*shape)
    ce_ref, target_ref, g_ref = oracle(inp)
    x = _fp64(inp)
    ce, target = L.c51_td_cross_entropy(
        x["lt1"], x["z_tm1"], x["a"], x["r"], x["d"], x["lt"], x["z_t"], x["sel"],
        return_target=True,
    )
    assert ce.dtype == torch.float64 and not target.requires_grad
    (g,) = torch.autograd.grad(ce.sum(), x["lt1"])
    torch.testing.assert_close(ce.detach(), ce_ref, **TOL)
    torch.testing.assert_close(target, target_ref, **TOL)
    torch.testing.assert_close(g, g_ref, **TOL)


def test_c51_backward_scales_with_grad_ce_and_is_zero_off_action():
    inp = make_inputs(67, 3, 51, 51, seed=3)
    _, _, g_ref = oracle(inp)
    x = _fp64(inp)
    ce = L.c51_td_cross_entropy(
        x["lt1"], x["z_tm1"], x["a"], x["r"], x["d"], x["lt"], x["z_t"], x["sel"]
    )
    w = torch.linspace(0.5, 2.0, 67, dtype=torch.float64)
    (g,) = torch.autograd.grad((w * ce).sum(), x["lt1"])
    torch.testing.assert_close(g, w.view(-1, 1, 1) * g_ref, **TOL)
    taken = torch.zeros(67, 3, dtype=torch.bool)
    taken[torch.arange(67), inp["a"]] = True
    assert (g[~taken] == 0).all()


def test_c51_2d_form_equals_3d_form_with_one_action():
    inp = make_inputs(9, 1, 5, 5)
    x = _fp64(inp)
    ce3, t3 = L.c51_td_cross_entropy(
        x["lt1"], x["z_tm1"], x["a"], x["r"], x["d"], x["lt"], x["z_t"], x["sel"],
        return_target=True,
    )
    lt1_2d = x["lt1"].detach()[:, 0].clone().requires_grad_(True)
    ce2, t2 = L.c51_td_cross_entropy(
        lt1_2d, x["z_tm1"], None, x["r"], x["d"], x["lt"][:, 0], x["z_t"],
        return_target=True,
    )
    assert torch.equal(ce2, ce3) and torch.equal(t2, t3)
    (g3,) = torch.autograd.grad(ce3.sum(), x["lt1"])
    (g2,) = torch.autograd.grad(ce2.sum(), lt1_2d)
    assert g2.shape == (9, 5) and torch.equal(g2, g3[:, 0])


def test_c51_bad_action_gives_nan_ce_and_zero_grad():
    inp = make_inputs(9, 3, 5, 5)
    inp["a"][2], inp["a"][6] = 3, -1
    x = _fp64(inp)
    ce = L.c51_td_cross_entropy(
        x["lt1"], x["z_tm1"], x["a"], x["r"], x["d"], x["lt"], x["z_t"], x["sel"]
    )
    bad = torch.zeros(9, dtype=torch.bool)
    bad[[2, 6]] = True
    assert ce[bad].isnan().all() and ce[~bad].isfinite().all()
    (g,) = torch.autograd.grad(ce[~bad].sum() + ce[bad].sum(), x["lt1"])
    assert (g[bad] == 0).all() and g[~bad].abs().sum() > 0


def test_c51_knob_off_and_per_row_atoms_run_the_torch_composition(monkeypatch):
    inp = make_inputs(11, 2, 51, 33)
    ce_ref, _, _ = oracle(inp)
    x = _fp64(inp)
    args = (x["lt1"], x["z_tm1"], x["a"], x["r"], x["d"], x["lt"], x["z_t"], x["sel"])
    calls = []
    real = L.categorical_l2_project
    monkeypatch.setattr(
        L, "categorical_l2_project", lambda *a: calls.append(1) or real(*a)
    )
    L.c51_td_cross_entropy(*args)
    assert not calls  # closed-form path
    # genuinely per-row supports are not one support: composition
    z_rows = x["z_t"].unsqueeze(0).repeat(11, 1)
    ce = L.c51_td_cross_entropy(*args[:6], z_rows, x["sel"])
    assert len(calls) == 1
    torch.testing.assert_close(ce.detach(), ce_ref, **TOL)
    # an expanded view of one row is one support
    L.c51_td_cross_entropy(*args[:6], x["z_t"].unsqueeze(0).expand(11, -1), x["sel"])
    assert len(calls) == 1
    monkeypatch.setenv("STOIX_FUSED_C51", "0")
    ce = L.c51_td_cross_entropy(*args)
    assert len(calls) == 2
    torch.testing.assert_close(ce.detach(), ce_ref, **TOL)


def test_categorical_losses_unchanged_on_cpu():
    inp = make_inputs(11, 2, 51, 33)
    ce_ref, _, _ = oracle(inp)
    x = _fp64(inp)
    out = L.categorical_double_q_learning(
        x["lt1"], x["z_tm1"], x["a"], x["r"], x["d"], x["lt"], x["z_t"], x["sel"]
    )
    assert torch.equal(out.detach(), ce_ref.mean())
    # the 2-D loss: same assembly with the action axis taken out
    one = make_inputs(9, 1, 5, 5)
    ce_ref, _, _ = oracle(one)
    y = _fp64(one)
    out = L.categorical_td_learning(
        y["lt1"][:, 0], y["z_tm1"], y["r"], y["d"], y["lt"][:, 0], y["z_t"]
    )
    assert torch.equal(out.detach(), ce_ref.mean())
