"""GPU tests of the fused C51 loss kernels (ops/csrc/c51.hip) against the
fp64 CPU assembly in c51_oracle.py, fed the same inputs (for bf16 logits:
the bf16-rounded inputs, upcast).

Tolerances: fp32 outputs rtol = atol = 1e-4, the project's fp32
kernel-vs-CPU tolerance; the bf16 gradient rtol = 2**-8 (twice one bf16
rounding) with atol = 1e-4; mass within M * 2**-23.
"""
import pytest
import torch

from c51_oracle import make_inputs, oracle, to_device

pytestmark = pytest.mark.gpu

requires_gpu = pytest.mark.skipif(not torch.cuda.is_available(), reason="no GPU")

# row tail + atoms below one wave; 2-D form, tiny support, B < 64; three lane
# passes with a ragged last one; N != M
SHAPES = [(67, 3, 51, 51), (9, 1, 5, 5), (13, 4, 130, 130), (11, 2, 51, 33)]
FP32_TOL = dict(rtol=1e-4, atol=1e-4)


def _run(inp, two_d=False):
    """(ce, target, dlogits for grad_ce = ones) from the CUDA path."""
    from stoix_amd.ops import losses as L

    x = to_device(inp, "cuda")
    if two_d:
        lt1 = x["lt1"][:, 0].contiguous().requires_grad_(True)
        args = (lt1, x["z_tm1"], None, x["r"], x["d"], x["lt"][:, 0].contiguous(), x["z_t"], None)
    else:
        lt1 = x["lt1"].requires_grad_(True)
        args = (lt1, x["z_tm1"], x["a"], x["r"], x["d"], x["lt"], x["z_t"], x["sel"])
    ce, target = L.c51_td_cross_entropy(*args, return_target=True)
    (g,) = torch.autograd.grad(ce.sum(), lt1)
    if two_d:
        g = g.unsqueeze(1)
    return ce.detach(), target, g


@pytest.fixture(scope="module")
def cases():
    """Per shape: inputs, the fp64 oracle and one kernel run, computed once."""
    from stoix_amd import ops

    assert ops.ext(required=True) is not None
    out = {}
    for shape in SHAPES:
        inp = make_inputs(*shape)
        out[shape] = (inp, oracle(inp), _run(inp, two_d=shape[1] == 1))
    return out


@requires_gpu
@pytest.mark.parametrize("shape", SHAPES)
def test_c51_fp32_matches_fp64_oracle(cases, shape):
    _, (ce_ref, t_ref, g_ref), (ce, target, g) = cases[shape]
    assert ce.dtype == target.dtype == g.dtype == torch.float32
    ce, target, g = ce.cpu().double(), target.cpu().double(), g.cpu().double()
    print(
        f"{shape}: max abs err ce {(ce - ce_ref).abs().max():.3e} "
        f"target {(target - t_ref).abs().max():.3e} dlogits {(g - g_ref).abs().max():.3e}"
    )
    torch.testing.assert_close(ce, ce_ref, **FP32_TOL)
    torch.testing.assert_close(target, t_ref, **FP32_TOL)
    torch.testing.assert_close(g, g_ref, **FP32_TOL)


@requires_gpu
def test_c51_bf16_logits_match_fp64_oracle_on_rounded_inputs():
    inp = make_inputs(67, 3, 51, 51, seed=1, dtype=torch.bfloat16)
    ce_ref, t_ref, g_ref = oracle(inp)  # upcasts the bf16-rounded logits
    ce, target, g = _run(inp)
    assert ce.dtype == target.dtype == torch.float32 and g.dtype == torch.bfloat16
    ce, target, g = ce.cpu().double(), target.cpu().double(), g.cpu().double()
    print(
        f"bf16: max abs err ce {(ce - ce_ref).abs().max():.3e} "
        f"target {(target - t_ref).abs().max():.3e} dlogits {(g - g_ref).abs().max():.3e}"
    )
    torch.testing.assert_close(ce, ce_ref, **FP32_TOL)
    torch.testing.assert_close(target, t_ref, **FP32_TOL)
    torch.testing.assert_close(g, g_ref, rtol=2.0**-8, atol=1e-4)


@requires_gpu
@pytest.mark.parametrize("shape", SHAPES)
def test_c51_target_keeps_the_mass(cases, shape):
    _, _, (_, target, _) = cases[shape]
    M = shape[3]
    assert (target >= 0).all()
    err = (target.cpu().double().sum(-1) - 1.0).abs()
    print(f"{shape}: max |sum(target) - 1| = {err.max():.3e} (bound {M * 2.0**-23:.3e})")
    assert err.max() <= M * 2.0**-23  # edge rows included


@requires_gpu
def test_c51_gradient_is_exactly_zero_off_the_taken_action(cases):
    # another shape first, so the allocator hands the gradient used memory
    _run(make_inputs(13, 4, 130, 130, seed=5))
    inp = make_inputs(67, 3, 51, 51, seed=6)
    _, _, g = _run(inp)
    taken = torch.zeros(67, 3, dtype=torch.bool)
    taken[torch.arange(67), inp["a"]] = True
    g = g.cpu()
    assert (g[~taken] == 0).all()
    assert (g[taken].abs().sum(-1) > 0).all()


@requires_gpu
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_c51_is_deterministic(dtype):
    inp = make_inputs(67, 3, 51, 51, seed=2, dtype=dtype)
    first, second = _run(inp), _run(inp)
    for x, y in zip(first, second):
        assert torch.equal(x, y)


@requires_gpu
def test_c51_reads_strided_row_vectors_in_place(cases):
    # a/r/d as columns of [B, 3] batches (the replay layout) and a weighted
    # gradient: same bits as the contiguous vectors
    from stoix_amd.ops import losses as L

    inp, _, (ce_ref, target_ref, g_ref) = cases[(67, 3, 51, 51)]
    x = to_device(inp, "cuda")
    cols = {k: torch.stack([x[k] + 1, x[k], x[k] - 1], dim=1)[:, 1] for k in ("a", "r", "d")}
    assert not cols["r"].is_contiguous()
    lt1 = x["lt1"].requires_grad_(True)
    ce, target = L.c51_td_cross_entropy(
        lt1, x["z_tm1"], cols["a"], cols["r"], cols["d"], x["lt"], x["z_t"], x["sel"],
        return_target=True,
    )
    (g,) = torch.autograd.grad(ce.sum(), lt1)
    assert torch.equal(ce.detach(), ce_ref) and torch.equal(target, target_ref)
    assert torch.equal(g, g_ref)


@requires_gpu
def test_c51_bad_action_is_in_bounds_nan_ce_zero_grad():
    inp = make_inputs(9, 3, 5, 5)
    inp["a"][2], inp["a"][6] = 3, -1
    ce, target, g = _run(inp)
    bad = torch.zeros(9, dtype=torch.bool)
    bad[[2, 6]] = True
    ce, g = ce.cpu(), g.cpu()
    assert ce[bad].isnan().all() and ce[~bad].isfinite().all()
    assert (g[bad] == 0).all() and target.isfinite().all()


@requires_gpu
def test_categorical_losses_route_to_the_kernel(cases, monkeypatch):
    from stoix_amd.ops import losses as L

    def boom(*a, **k):
        raise RuntimeError("torch projection called")

    monkeypatch.setattr(L, "categorical_l2_project", boom)
    inp, (ce_ref, _, _), _ = cases[(67, 3, 51, 51)]
    x = to_device(inp, "cuda")
    dq = (x["lt1"], x["z_tm1"], x["a"], x["r"], x["d"], x["lt"], x["z_t"], x["sel"])
    out = L.categorical_double_q_learning(*dq)
    torch.testing.assert_close(out.cpu().double(), ce_ref.mean(), **FP32_TOL)
    # per-row atoms that are an expanded view of one row still qualify
    out = L.categorical_double_q_learning(
        x["lt1"], x["z_tm1"].unsqueeze(0).expand(67, -1), x["a"], x["r"], x["d"],
        x["lt"], x["z_t"].unsqueeze(0).expand(67, -1), x["sel"],
    )
    torch.testing.assert_close(out.cpu().double(), ce_ref.mean(), **FP32_TOL)
    inp1, (ce_ref1, _, _), _ = cases[(9, 1, 5, 5)]
    y = to_device(inp1, "cuda")
    td = (y["lt1"][:, 0], y["z_tm1"], y["r"], y["d"], y["lt"][:, 0], y["z_t"])
    out = L.categorical_td_learning(*td)
    torch.testing.assert_close(out.cpu().double(), ce_ref1.mean(), **FP32_TOL)
    monkeypatch.setenv("STOIX_FUSED_C51", "0")
    with pytest.raises(RuntimeError, match="torch projection called"):
        L.categorical_double_q_learning(*dq)
    with pytest.raises(RuntimeError, match="torch projection called"):
        L.categorical_td_learning(*td)


@requires_gpu
def test_c51_forward_backward_graph_capture():
    from stoix_amd.ops import losses as L

    B, A, N, M = 64, 4, 51, 51
    static = to_device(make_inputs(B, A, N, M, seed=10), "cuda")
    static["lt1"].requires_grad_(True)

    def step(x):
        ce, target = L.c51_td_cross_entropy(
            x["lt1"], x["z_tm1"], x["a"], x["r"], x["d"], x["lt"], x["z_t"], x["sel"],
            return_target=True,
        )
        (g,) = torch.autograd.grad(ce.sum(), x["lt1"])
        return ce.detach(), target, g

    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        step(static)
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        outs = step(static)
    fresh = to_device(make_inputs(B, A, N, M, seed=11), "cuda")
    with torch.no_grad():
        for k, v in fresh.items():
            static[k].copy_(v)
    graph.replay()
    fresh["lt1"].requires_grad_(True)
    eager = step(fresh)
    torch.cuda.synchronize()
    for x, y in zip(outs, eager):
        assert torch.equal(x, y)


@requires_gpu
def test_ineligible_per_row_atoms_fall_back_to_torch(cases, monkeypatch):
    from stoix_amd.ops import losses as L

    inp, (ce_ref, _, _), _ = cases[(11, 2, 51, 33)]
    x = to_device(inp, "cuda")
    calls = []
    real = L.categorical_l2_project
    monkeypatch.setattr(L, "categorical_l2_project", lambda *a: calls.append(1) or real(*a))
    out = L.categorical_double_q_learning(
        x["lt1"], x["z_tm1"].unsqueeze(0).repeat(11, 1), x["a"], x["r"], x["d"],
        x["lt"], x["z_t"].unsqueeze(0).repeat(11, 1), x["sel"],
    )
    assert calls  # the torch composition ran
    torch.testing.assert_close(out.cpu().double(), ce_ref.mean(), **FP32_TOL)
