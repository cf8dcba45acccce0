"""GPU tests for wgrad_pair_act (wgrad_pair_act_kernel in
stoix_amd/ops/csrc/wgrad.hip): the layer-1 paired wgrad that forms
dZ = bf16(dH * silu'(Z)) while it stages its tiles, so that the engine needs
neither the layer-1 silu_bwd launch nor the dZ1 buffer (STOIX_FUSED_DZ1).
The contract is raw-bit equality of every slab element with silu_bwd +
wgrad_pair on the same operands, and that a call which is not taken
launches nothing."""
import functools

import pytest
import torch

pytestmark = pytest.mark.gpu

requires_gpu = pytest.mark.skipif(not torch.cuda.is_available(), reason="no GPU")

BF16_MAX = 3.3895313892515355e38  # largest finite bf16
GUARD = 12345.0  # slab sentinel; no sum of these operands gives it


@pytest.fixture(scope="module")
def ext():
    from stoix_amd import ops

    e = ops.ext(required=True)
    assert e is not None
    return e


def _n_slices(S):
    n = 64
    while n > 4 and S % (32 * n) != 0:
        n //= 2
    return n


@functools.lru_cache(maxsize=None)
def _operands(S, N, K):
    """Stacked [2, S, N] dH and Z, as the engine holds them, and one shared X.
    Z covers [-20, 20] densely (every bf16 value in it, cycled), with +-0,
    +-88, +-1e4 and +-the largest finite bf16 mixed in: around -88 __expf
    overflows and silu' goes through inf / NaN, which both paths must do
    alike. dH has zeros and both signs. Never written to."""
    g = torch.Generator().manual_seed(4200 + 7 * S + 3 * N + K)
    allbf = torch.arange(-32768, 32768, dtype=torch.int32).to(torch.int16).view(torch.bfloat16)
    dense = allbf[allbf.float().abs() <= 20.0]
    special = torch.tensor([0.0, -0.0, 88.0, -88.0, 1e4, -1e4, BF16_MAX, -BF16_MAX,
                            87.0, -87.0, 89.0, -89.0, 100.0, -100.0]).bfloat16()
    pool = torch.cat([dense, special.repeat(64)])
    n = 2 * S * N
    pick = torch.randint(0, pool.numel(), (n,), generator=g)
    Z = pool[pick].view(2, S, N).contiguous()
    dH = (torch.randn(2, S, N, generator=g) * 0.1).bfloat16()
    dH[torch.rand(2, S, N, generator=g) < 0.1] = 0.0
    X = torch.randn(S, K, generator=g).bfloat16()
    return dH.cuda(), Z.cuda(), X.cuda()


def _layout(K, N):
    dW = [8, 40]
    db = [8 + N * K + 24, 40 + N * K + 8]
    stride = max(db[0] + N, db[1] + N) + 64
    return dW, db, stride


def _slabs(stride):
    return [torch.full((64, stride), GUARD, dtype=torch.float32, device="cuda")
            for _ in range(2)]


@functools.lru_cache(maxsize=None)
def _reference(S, N, K):
    """Slabs of silu_bwd + wgrad_pair, computed once per shape."""
    from stoix_amd import ops

    e = ops.ext(required=True)
    dH, Z, X = _operands(S, N, K)
    dW, db, stride = _layout(K, N)
    dZ = torch.empty_like(dH)
    e.silu_bwd(dH, Z, dZ)
    slabs = _slabs(stride)
    assert e.wgrad_pair(dZ[0], X, slabs[0], dW[0], db[0], N,
                        dZ[1], X, slabs[1], dW[1], db[1], N) is True
    torch.cuda.synchronize()
    return slabs, dZ


def _act(ext, dH, Z, X, slabs, dW, db, N, **kw):
    return ext.wgrad_pair_act(dH[0], Z[0], X, slabs[0], dW[0], db[0], N,
                              dH[1], Z[1], X, slabs[1], dW[1], db[1], N, **kw)


def _i32(t):
    return t.view(torch.int32)


# S = 256: 8 slices of one 32-row step (a half-filled stage at two steps a
# stage); 4096: 64 slices, exactly one stage; 6144: a full plus a partial stage
@requires_gpu
@pytest.mark.parametrize("S", [256, 4096, 6144])
@pytest.mark.parametrize("N", [128, 256])
@pytest.mark.parametrize("K", [32, 64, 96])
def test_fused_slab_is_bit_equal(ext, S, N, K):
    """dW and db of both nets, compared as int32 so that NaNs cannot hide a
    difference; exactly the elements the plain pair writes are written."""
    dH, Z, X = _operands(S, N, K)
    ref, dZ = _reference(S, N, K)
    dW, db, stride = _layout(K, N)
    new = _slabs(stride)
    assert _act(ext, dH, Z, X, new, dW, db, N) is True
    torch.cuda.synchronize()
    ns = _n_slices(S)
    for i in range(2):
        written = torch.zeros(64, stride, dtype=torch.bool, device="cuda")
        written[:ns, dW[i]: dW[i] + N * K] = True
        written[:ns, db[i]: db[i] + N] = True
        assert (ref[i][~written] == GUARD).all(), "mask misses a reference write"
        assert torch.equal(_i32(new[i]), _i32(ref[i])), f"net {i}"
        assert not (new[i][written] == GUARD).all()
    # the inputs do reach the overflow region, and the nets differ
    assert not torch.isfinite(dZ.float()).all() or (Z.float() < -88).any()
    assert not torch.equal(_i32(new[0][:, dW[0]: dW[0] + N * K]),
                           _i32(new[1][:, dW[1]: dW[1] + N * K]))


@requires_gpu
def test_one_step_a_stage_variant_is_bit_equal(ext):
    """The SB = 1 tile of K = 32 that the sweep compares (variant 1)."""
    S, N, K = 6144, 256, 32
    dH, Z, X = _operands(S, N, K)
    ref, _ = _reference(S, N, K)
    dW, db, stride = _layout(K, N)
    new = _slabs(stride)
    assert _act(ext, dH, Z, X, new, dW, db, N, variant=1) is True
    torch.cuda.synchronize()
    for i in range(2):
        assert torch.equal(_i32(new[i]), _i32(ref[i]))


@requires_gpu
def test_refusals_leave_the_slab_alone(ext):
    S, N, K = 256, 128, 32
    dH, Z, X = _operands(S, N, K)
    dW, db, stride = _layout(K, N)
    slabs = _slabs(stride)
    none = torch.zeros(0, dtype=torch.bfloat16, device="cuda")

    def call(Z0=Z[0], Z1=Z[1], X_=X, dW_=dW, db_=db, st=slabs):
        return ext.wgrad_pair_act(dH[0], Z0, X_, st[0], dW_[0], db_[0], N,
                                  dH[1], Z1, X_, st[1], dW_[1], db_[1], N)

    # Z on one net only: not taken
    assert call(Z1=none) is False
    assert call(Z0=none) is False
    assert call(Z0=none, Z1=none) is False
    with pytest.raises(RuntimeError, match="dtype"):
        call(Z0=Z[0].float())
    with pytest.raises(RuntimeError, match="shape"):
        call(Z0=Z[0][:128].contiguous())
    with pytest.raises(RuntimeError, match="shape"):
        call(Z1=torch.zeros(S, N + 16, dtype=torch.bfloat16, device="cuda"))
    with pytest.raises(RuntimeError, match="contiguous"):
        call(Z0=torch.zeros(N, S, dtype=torch.bfloat16, device="cuda").t())
    # K outside the layer-1 table: not taken, nothing launched
    K2 = 256
    X2 = torch.zeros(S, K2, dtype=torch.bfloat16, device="cuda")
    dW2, db2, stride2 = _layout(K2, N)
    big = _slabs(stride2)
    assert call(X_=X2, dW_=dW2, db_=db2, st=big) is False
    torch.cuda.synchronize()
    for s in slabs + big:
        assert (s == GUARD).all()


@requires_gpu
def test_three_graph_replays_give_the_same_bits(ext):
    S, N, K = 6144, 256, 32
    dH, Z, X = _operands(S, N, K)
    ref, _ = _reference(S, N, K)
    dW, db, stride = _layout(K, N)
    slabs = _slabs(stride)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        assert _act(ext, dH, Z, X, slabs, dW, db, N) is True  # warm-up
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        _act(ext, dH, Z, X, slabs, dW, db, N)
    for _ in range(3):
        for s in slabs:
            s.fill_(GUARD)
        graph.replay()
        torch.cuda.synchronize()
        for i in range(2):
            assert torch.equal(_i32(slabs[i]), _i32(ref[i]))
