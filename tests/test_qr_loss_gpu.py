"""GPU tests of the fused QR loss kernels (ops/csrc/qr.hip) against the fp64
CPU composition in qr_oracle.py, fed the same inputs (for bf16: the
bf16-rounded inputs, upcast).

Tolerances: fp32 outputs rtol = atol = 1e-4, the project's fp32
kernel-vs-CPU tolerance (FP32_TOL of test_c51_loss_gpu.py); the bf16
gradient rtol = 2**-8 (twice one bf16 rounding) with atol = 1e-4.
"""
import pytest
import torch

from qr_oracle import make_inputs, oracle, to_device

pytestmark = pytest.mark.gpu

requires_gpu = pytest.mark.skipif(not torch.cuda.is_available(), reason="no GPU")

# row tail + N below one wave; A = 1, B below a wave; four lane passes with a
# ragged last one; N != M with M below a wave
SHAPES = [(67, 3, 51, 51), (9, 1, 5, 5), (13, 4, 200, 200), (11, 2, 130, 33)]
HUBER = [1.0, 0.5, 0.0]
FP32_TOL = dict(rtol=1e-4, atol=1e-4)
KEYS = ("src", "tau", "a", "r", "d", "sel", "tgt")


def _run(x, k, weight=None):
    """(loss [B], dsrc for a gradient of ones or ``weight``) from device inputs."""
    from stoix_amd.ops import losses as L

    src = x["src"].detach().requires_grad_(True)
    loss = L.quantile_q_learning_rows(src, *(x[n] for n in KEYS[1:]), k)
    (g,) = torch.autograd.grad(loss.sum() if weight is None else (weight * loss).mean(), src)
    return loss.detach(), g


@pytest.fixture(scope="module")
def cases():
    """Per (shape, k): inputs, the fp64 oracle and one kernel run, computed once."""
    from stoix_amd import ops

    assert hasattr(ops.ext(required=True), "qr_loss_fwd")
    out = {}
    for shape in SHAPES:
        inp = make_inputs(*shape)
        for k in HUBER:
            out[shape, k] = (inp, oracle(inp, k), _run(to_device(inp, "cuda"), k))
    return out


@requires_gpu
@pytest.mark.parametrize("k", HUBER)
@pytest.mark.parametrize("shape", SHAPES)
def test_qr_fp32_matches_fp64_oracle(cases, shape, k):
    _, (loss_ref, g_ref), (loss, g) = cases[shape, k]
    assert loss.dtype == g.dtype == torch.float32
    loss, g = loss.cpu().double(), g.cpu().double()
    print(
        f"{shape} k={k}: max abs err loss {(loss - loss_ref).abs().max():.3e} "
        f"(|loss| up to {loss_ref.abs().max():.3e}) dsrc {(g - g_ref).abs().max():.3e}"
    )
    torch.testing.assert_close(loss, loss_ref, **FP32_TOL)
    torch.testing.assert_close(g, g_ref, **FP32_TOL)


@requires_gpu
def test_qr_bf16_matches_fp64_oracle_on_rounded_inputs():
    inp = make_inputs(67, 3, 51, 51, seed=1, dtype=torch.bfloat16)
    loss_ref, g_ref = oracle(inp, 1.0)  # upcasts the bf16-rounded inputs
    loss, g = _run(to_device(inp, "cuda"), 1.0)
    assert loss.dtype == torch.float32 and g.dtype == torch.bfloat16
    loss, g = loss.cpu().double(), g.cpu().double()
    print(
        f"bf16: max abs err loss {(loss - loss_ref).abs().max():.3e} "
        f"dsrc {(g - g_ref).abs().max():.3e}"
    )
    torch.testing.assert_close(loss, loss_ref, **FP32_TOL)
    torch.testing.assert_close(g, g_ref, rtol=2.0**-8, atol=1e-4)


@requires_gpu
def test_qr_gradient_is_exactly_zero_off_the_taken_action():
    # another shape first, so the allocator hands the gradient used memory
    _run(to_device(make_inputs(13, 4, 200, 200, seed=5), "cuda"), 1.0)
    inp = make_inputs(67, 3, 51, 51, seed=6)
    _, g = _run(to_device(inp, "cuda"), 1.0)
    taken = torch.zeros(67, 3, dtype=torch.bool)
    taken[torch.arange(67), inp["a"]] = True
    g = g.cpu().transpose(1, 2)  # [B, A, N]
    assert (g[~taken] == 0).all()
    assert (g[taken].abs().sum(-1) > 0).all()


@requires_gpu
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_qr_is_deterministic(dtype):
    x = to_device(make_inputs(13, 4, 200, 200, seed=2, dtype=dtype), "cuda")
    first, second = _run(x, 1.0), _run(x, 1.0)
    for u, v in zip(first, second):
        assert torch.equal(u, v)


@requires_gpu
def test_qr_reads_strided_row_vectors_and_tau_in_place(cases):
    # a/r/d as columns of [B, 3] batches (the replay layout), tau as an
    # expanded [B, N] view and a weighted gradient: same bits as contiguous
    inp, _, (loss_ref, _) = cases[(67, 3, 51, 51), 1.0]
    x = to_device(inp, "cuda")
    w = torch.linspace(0.5, 2.0, 67, device="cuda")
    _, g_ref = _run(x, 1.0, weight=w)
    y = dict(x, tau=x["tau"].unsqueeze(0).expand(67, -1))
    for n in ("a", "r", "d"):
        y[n] = torch.stack([x[n] + 1, x[n], x[n] - 1], dim=1)[:, 1]
    assert not y["r"].is_contiguous() and y["tau"].stride(0) == 0
    loss, g = _run(y, 1.0, weight=w)
    assert torch.equal(loss, loss_ref) and torch.equal(g, g_ref)


@requires_gpu
def test_quantile_losses_route_to_the_kernel(cases, monkeypatch):
    from stoix_amd.ops import losses as L

    def boom(*a, **k):
        raise RuntimeError("torch huber called")

    monkeypatch.setattr(L, "_huber", boom)
    inp, (loss_ref, _), _ = cases[(67, 3, 51, 51), 1.0]
    x = to_device(inp, "cuda")
    args = tuple(x[n] for n in KEYS)
    out = L.quantile_q_learning(*args, 1.0)
    torch.testing.assert_close(out.cpu().double(), loss_ref.mean(), **FP32_TOL)
    # the 2-D loss on a target formed beforehand: A = 1 in the kernel
    one, (loss_ref1, g_ref1), _ = cases[(9, 1, 5, 5), 1.0]
    y = to_device(one, "cuda")
    src2 = y["src"][:, :, 0].clone().requires_grad_(True)
    target = y["r"].unsqueeze(-1) + y["d"].unsqueeze(-1) * y["tgt"][:, :, 0]
    out2 = L.quantile_regression_loss(src2, y["tau"], target, 1.0)
    (g2,) = torch.autograd.grad(out2, src2)
    torch.testing.assert_close(out2.detach().cpu().double(), loss_ref1.mean(), **FP32_TOL)
    torch.testing.assert_close(9 * g2.cpu().double(), g_ref1[:, :, 0], **FP32_TOL)
    monkeypatch.setenv("STOIX_FUSED_QR", "0")
    with pytest.raises(RuntimeError, match="torch huber called"):
        L.quantile_q_learning(*args, 1.0)
    with pytest.raises(RuntimeError, match="torch huber called"):
        L.quantile_regression_loss(src2, y["tau"], target, 1.0)


@requires_gpu
def test_qr_forward_backward_graph_capture():
    shape = (64, 4, 200, 51)
    static = to_device(make_inputs(*shape, seed=10), "cuda")
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        _run(static, 1.0)
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        outs = _run(static, 1.0)
    for seed in (11, 12):  # several replays, each against eager
        fresh = to_device(make_inputs(*shape, seed=seed), "cuda")
        for n, v in fresh.items():
            static[n].copy_(v)
        graph.replay()
        eager = _run(fresh, 1.0)
        torch.cuda.synchronize()
        for u, v in zip(outs, eager):
            assert torch.equal(u, v)
