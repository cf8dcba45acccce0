"""Tests for the two-launch optimiser tail of the fused PPO engine
(STOIX_FUSED_TAIL): slab_reduce_norm_pair (stoix_amd/ops/csrc/wgrad.hip) +
adam_pair (optim.hip) against the sequence they replace, slab_reduce_pair +
fused_adam_bf16 per chain with the ordered-partials sqnorm buffer. The
contract is bit-equality of everything both sequences leave behind, which
for sqnorm[0] means one fixed order of float adds (ordered_sqnorm below
spells it out in NumPy)."""
import functools

import numpy as np
import pytest
import torch

requires_gpu = pytest.mark.skipif(not torch.cuda.is_available(), reason="no GPU")

MAX_NORM = 0.5
HYPER = (0.9, 0.999, 1e-5, MAX_NORM)  # beta1, beta2, eps, max_grad_norm
SENTINEL = 7.0


def flagship_len(obs=27, H=256):
    """Elements of the actor chain of a 27-obs / 8-act, H = 256 engine: W1
    [H, K1P], b1, Wh [16, H], bh [16], b2, W2 [H, H] (fused.py a_specs)."""
    k1p = (obs + 31) & ~31
    return H * k1p + H + 16 * H + 16 + H + H * H


# --------------------------------------------------------- order of the adds


def _tree(a):
    """Lane 0 of `acc += __shfl_down(acc, off)` for off = 32..1 over the last
    axis (64 lanes), in float32."""
    a = a.astype(np.float32).copy()
    off = 32
    while off:
        a[..., :off] = a[..., :off] + a[..., off:2 * off]
        off //= 2
    return a[..., 0]


def ordered_sqnorm(x):
    """sqnorm[0] as the kernels form it, every add rounded to float32."""
    x = np.asarray(x, dtype=np.float32)
    n = x.size
    nvec = n // 8
    nb = max(1, -(-nvec // 256))  # blocks of the norm kernel, 256 groups each
    acc = np.zeros(nb * 256, dtype=np.float32)
    sq = x * x
    for j in range(8):  # ((0 + x0^2) + x1^2) + ... + x7^2 per group of 8
        acc[:nvec] = acc[:nvec] + sq[j:nvec * 8:8]
    tail = n - nvec * 8  # the n % 8 last elements go to groups 0..tail-1
    acc[:tail] = acc[:tail] + sq[nvec * 8:]
    waves = _tree(acc.reshape(nb, 4, 64))  # one tree per 64 groups
    part = np.zeros(nb, dtype=np.float32)
    for w in range(4):  # the four wave sums of a block, in order from 0
        part = part + waves[:, w]
    lanes = np.zeros(64, dtype=np.float32)
    for p0 in range(0, nb, 64):  # partials lane-strided by 64
        chunk = part[p0:p0 + 64]
        lanes[:chunk.size] = lanes[:chunk.size] + chunk
    return _tree(lanes)


def test_ordered_sum_is_within_the_float32_bound():
    """No GPU needed: the stated order of adds, emulated in float32, against
    a float64 sum at the flagship length. Every term is non-negative and each
    passes through fewer than n roundings, so the error stays within
    n * 2^-24 * sum(x^2)."""
    n = flagship_len()
    assert n % 8 == 0 and n % 256 != 0
    rng = np.random.default_rng(3)
    for m in (n, n + 5):  # the engine's length, and one with a tail
        x = (rng.standard_normal(m) * 0.01).astype(np.float32)
        got = float(ordered_sqnorm(x))
        want = float(np.sum(x.astype(np.float64) ** 2))
        assert abs(got - want) <= m * 2.0 ** -24 * want
        assert got != 0.0


# ------------------------------------------------------------------ GPU side


@pytest.fixture(scope="module")
def ext():
    from stoix_amd import ops

    e = ops.ext(required=True)
    assert e is not None
    return e


@functools.lru_cache(maxsize=None)
def _engine_lens():
    """(actor, critic) chain lengths of a small 27-obs / 8-act, H = 256
    fused engine: the flagship's chains."""
    from test_linear_silu_pair_gpu import _learner

    F_ = _learner("1", "1").fused
    return F_.actor_chain.flat.numel(), F_.critic_chain.flat.numel()


class _State:
    """Both chains' buffers for one of the two sequences."""

    def __init__(self, ns, scale, seed):
        g = torch.Generator().manual_seed(seed)
        self.ns = ns
        self.slab, self.grad16, self.p, self.m, self.v, self.p16 = [], [], [], [], [], []
        self.sqnorm, self.step, self.counter = [], [], []
        for i, n in enumerate(ns):
            stride = n + 24  # a slab image longer than the chain
            self.slab.append((torch.randn(64, stride, generator=g) * scale).cuda())
            self.grad16.append(torch.full((n,), SENTINEL, dtype=torch.bfloat16, device="cuda"))
            self.p.append(torch.randn(n, generator=g).cuda())
            self.m.append((torch.randn(n, generator=g) * 0.01).cuda())
            self.v.append((torch.rand(n, generator=g) * 1e-4).cuda())
            self.p16.append(torch.zeros(n, dtype=torch.bfloat16, device="cuda"))
            self.sqnorm.append(torch.full((1 + max(2048, -(-n // 512)) + 8,), SENTINEL,
                                          device="cuda"))
            self.step.append(torch.full((1,), 3 + i, dtype=torch.int64, device="cuda"))
            self.counter.append(torch.zeros(1, dtype=torch.int32, device="cuda"))
        self.lr = (3e-4, 1e-3)

    def compared(self):
        out = {}
        for i in range(2):
            out[f"grad16.{i}"] = self.grad16[i].view(torch.int16)
            out[f"sqnorm0.{i}"] = self.sqnorm[i][:1].view(torch.int32)
            out[f"step.{i}"] = self.step[i]
            out[f"param.{i}"] = self.p[i].view(torch.int32)
            out[f"m.{i}"] = self.m[i].view(torch.int32)
            out[f"v.{i}"] = self.v[i].view(torch.int32)
            out[f"param_bf16.{i}"] = self.p16[i].view(torch.int16)
        return {k: v.clone() for k, v in out.items()}


def _old(ext, s):
    ext.slab_reduce_pair(s.slab[0], s.grad16[0], s.sqnorm[0], s.step[0],
                         s.slab[1], s.grad16[1], s.sqnorm[1], s.step[1])
    for i in range(2):
        ext.fused_adam_bf16(s.p[i], s.grad16[i], s.m[i], s.v[i], s.sqnorm[i], s.step[i],
                            s.p16[i], s.lr[i], *HYPER, 1.0, 0)


def _new(ext, s):
    ext.slab_reduce_norm_pair(
        s.slab[0], s.grad16[0], s.sqnorm[0], s.step[0], s.counter[0],
        s.slab[1], s.grad16[1], s.sqnorm[1], s.step[1], s.counter[1])
    ext.adam_pair(s.p[0], s.grad16[0], s.m[0], s.v[0], s.sqnorm[0], s.step[0], s.p16[0],
                  s.lr[0], s.p[1], s.grad16[1], s.m[1], s.v[1], s.sqnorm[1], s.step[1],
                  s.p16[1], s.lr[1], *HYPER, 1.0)


def _assert_same(got, want, what):
    for k in want:
        assert torch.equal(got[k], want[k]), f"{what}: {k} differs"


def _scale(ns, clip):
    # a gradient element is the sum of 64 N(0, scale^2): norm ~ 8 * scale * sqrt(n)
    return 1.0 if clip else 0.02 / max(ns) ** 0.5


def _lens(name):
    if name == "flagship":
        return _engine_lens()
    return {
        "tiny": (5, 3),                  # n < 8: tail elements only
        "tail": (1023, 2048 * 3 + 5),    # n % 8 != 0, one just over whole blocks
        "ragged": (4104, 777),           # no multiples of 256 or 2048; 4104 % 8 == 0, 777 % 8 != 0
        "waves": (2056, 2048),           # a norm block with three empty waves
    }[name]


CASES = ["tiny", "tail", "ragged", "waves", "flagship"]


@pytest.mark.gpu
@requires_gpu
@pytest.mark.parametrize("clip", [True, False], ids=["clip", "noclip"])
@pytest.mark.parametrize("name", CASES)
def test_tail_is_bit_equal_over_three_calls(ext, name, clip):
    """Three consecutive calls on the same buffers: a counter that is not
    reset, or a stale partial, shows as a wrong sqnorm on the second."""
    ns = _lens(name)
    if name == "flagship":
        assert ns[0] == flagship_len()
    assert ns[0] != ns[1]
    old, new = _State(ns, _scale(ns, clip), 40), _State(ns, _scale(ns, clip), 40)
    for call in range(3):
        _old(ext, old)
        _new(ext, new)
        torch.cuda.synchronize()
        want = old.compared()
        _assert_same(new.compared(), want, f"{name} call {call}")
        for i, n in enumerate(ns):
            norm = float(new.sqnorm[i][0]) ** 0.5
            print(f"{name} chain {i}: n = {n}, norm = {norm:.4g}")
            assert (norm > MAX_NORM) == clip
            assert int(new.counter[i]) == 0
            assert int(new.step[i]) == 3 + i + call + 1
            used = 1 + -(-n // 512)
            assert (new.sqnorm[i][used:] == SENTINEL).all(), "wrote past the block sums"
            # the kernel's float is the one the stated order of adds gives
            g = new.grad16[i].float().cpu().numpy()
            assert np.float32(new.sqnorm[i][0].item()) == ordered_sqnorm(g)
        if call == 0:
            first = want
    # the calls did something: parameters moved between the first and third
    assert not torch.equal(first["param.0"], want["param.0"])


@pytest.mark.gpu
@requires_gpu
def test_tail_replays_from_a_graph(ext):
    """The tail runs inside the phase graphs: three replays of a captured
    slab_reduce_norm_pair + adam_pair against three eager old sequences."""
    ns = _lens("flagship")
    old, new = _State(ns, 1.0, 41), _State(ns, 1.0, 41)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        _new(ext, new)
    for call in range(3):
        _old(ext, old)
        graph.replay()
        torch.cuda.synchronize()
        _assert_same(new.compared(), old.compared(), f"replay {call}")
        assert all(int(c) == 0 for c in new.counter)


@pytest.mark.gpu
@requires_gpu
def test_tail_rejections(ext):
    s = _State((64, 64), 1.0, 42)
    with pytest.raises(RuntimeError, match="ceil"):
        ext.slab_reduce_norm_pair(
            torch.zeros(64, 4096, device="cuda"),
            torch.zeros(4096, dtype=torch.bfloat16, device="cuda"),
            torch.zeros(8, device="cuda"), s.step[0], s.counter[0],
            s.slab[1], s.grad16[1], s.sqnorm[1], s.step[1], s.counter[1])
    with pytest.raises(RuntimeError, match="dtype"):
        ext.slab_reduce_norm_pair(
            s.slab[0], s.grad16[0], s.sqnorm[0], s.step[0], s.counter[0].long(),
            s.slab[1], s.grad16[1], s.sqnorm[1], s.step[1], s.counter[1])
    with pytest.raises(RuntimeError, match="one length"):
        ext.adam_pair(s.p[0], s.grad16[0][:32], s.m[0], s.v[0], s.sqnorm[0], s.step[0],
                      s.p16[0], 1e-3, s.p[1], s.grad16[1], s.m[1], s.v[1], s.sqnorm[1],
                      s.step[1], s.p16[1], 1e-3, *HYPER, 1.0)
    assert int(ext.TAIL_MAX_N) == 2048 * 256 * 8
