"""GPU tests of the fused NoisyLinear kernels (ops/csrc/noisy.hip) against
fp64 on the CPU, computed from the operands the kernels are defined to see:
X and dZ rounded to bf16, W = bf16(mu + sigma * (eps_out x eps_in)) formed in
fp32 with torch ops, and, where a gradient passes through act', the bf16
pre-activation the forward stored.

Bounds (not measured): fp32 accumulation of exact bf16 products over a
reduction of length L is within L * 2**-23 of the sum of the absolute
products; one bf16 rounding (8 significant bits, to nearest) is within 2**-8
of the value, the project's bf16 rtol. Where dZ passed through act' outside
the test's reach, the reference rounds it to bf16 as well; the code forms
act' and the product in fp32 (within 2**-18 relative, a few ulp with margin),
so its rounding can fall on the other side only where the fp64 value lies
that close to a rounding boundary, and exactly there the bound allows one
bf16 ulp of that term (round_bf16).
"""
import math

import pytest
import torch

pytestmark = pytest.mark.gpu

requires_gpu = pytest.mark.skipif(not torch.cuda.is_available(), reason="no GPU")

# row tail, K below one k-step and no multiple of 32, N no multiple of 16;
# second row tile ragged, ragged K tail after full steps, N over tile
# boundaries; every tile full; Rainbow's layer-1 K with S below one tile; two
# wgrad slices of 160 rows, the second ragged (140 rows = 4 steps + 12)
SHAPES = [(67, 40, 51), (130, 72, 204), (256, 256, 256), (19, 720, 256), (300, 40, 51)]
E8, E23 = 2.0**-8, 2.0**-23


@pytest.fixture(autouse=True)
def fused_on(monkeypatch):
    monkeypatch.setenv("STOIX_FUSED_NOISY", "1")


def make_inputs(S, K, N):
    g = torch.Generator().manual_seed(1000 * S + 10 * K + N)

    def r(*shape):
        return torch.randn(*shape, generator=g)

    def eps(n):  # f(x) = sign(x) sqrt(|x|): non-zero, both signs
        e = r(n)
        return e.sign() * e.abs().sqrt()

    s = 1.0 / math.sqrt(K)
    return dict(x=r(S, K), mu_w=r(N, K) * s, sigma_w=r(N, K) * s, mu_b=r(N) * 0.1,
                sigma_b=r(N) * 0.1, eps_in=eps(K), eps_out=eps(N), gw=r(S, N))


def make_layer(inp):
    from stoix_amd.networks.layers import NoisyLinear

    N, K = inp["mu_w"].shape
    lin = NoisyLinear(K, N)
    with torch.no_grad():
        lin.weight_mu.copy_(inp["mu_w"])
        lin.weight_sigma.copy_(inp["sigma_w"])
        lin.bias_mu.copy_(inp["mu_b"])
        lin.bias_sigma.copy_(inp["sigma_b"])
    lin.eps_in, lin.eps_out = inp["eps_in"].clone(), inp["eps_out"].clone()
    return lin.cuda()


def ref_weight(inp, noisy=True):
    """(W, b, eps_out x eps_in) in fp64, W from its bf16 image."""
    e = torch.outer(inp["eps_out"], inp["eps_in"])
    if not noisy:
        return inp["mu_w"].bfloat16().double(), inp["mu_b"].double(), e.double()
    w = (inp["mu_w"] + inp["sigma_w"] * e).bfloat16().double()
    return w, (inp["mu_b"] + inp["sigma_b"] * inp["eps_out"]).double(), e.double()


def act_ref(z, act):
    """(act(z), act'(z)) in fp64."""
    if act == "silu":
        s = torch.sigmoid(z)
        return z * s, s * (1 + z * (1 - s))
    if act == "relu":
        return z.clamp(min=0), (z > 0).double()
    return z, torch.ones_like(z)


def round_bf16(v, delta=2.0**-18):
    """(bf16(v), slack) in fp64: slack is one bf16 ulp where an evaluation of
    v within delta relative could round the other way, else 0."""
    r = v.float().bfloat16().double()
    half = torch.exp2(torch.floor(torch.log2(v.abs().clamp(min=1e-300))) - 8)
    near = (half - (v - r).abs()) <= delta * v.abs()
    return r, torch.where(near & (v != 0), 2 * half, torch.zeros_like(v))


def within(got, ref, bound, what):
    err = (got.detach().cpu().double() - ref).abs()
    print(f"  {what}: max err {err.max():.3e}, max err/bound {(err / bound.clamp(min=1e-300)).max():.3f}")
    assert (err <= bound).all(), what


def run_layer(inp, x_dtype, act, noisy=True):
    """Forward through the module and gradients of sum(out * gw), plus a second
    fused apply for the stored pre-activation."""
    from stoix_amd.ops.noisy import noisy_linear_fused

    lin = make_layer(inp)
    lin.use_noise = noisy
    x = inp["x"].to(x_dtype).cuda().requires_grad_(True)
    params = [lin.weight_mu, lin.weight_sigma, lin.bias_mu, lin.bias_sigma]
    with torch.autocast("cuda", torch.bfloat16):
        out = lin(x, act=act)
        out2, pre = noisy_linear_fused(lin, x, act)
    grads = torch.autograd.grad((out.float() * inp["gw"].cuda()).sum(), [x] + params, allow_unused=True)
    return out, out2, (pre[0] if pre else out), grads


CASES = [(s, d, a) for s in SHAPES for d in (torch.float32, torch.bfloat16) for a in (None, "silu")]
CASES.append((SHAPES[0], torch.float32, "relu"))


@requires_gpu
@pytest.mark.parametrize("shape,x_dtype,act", CASES)
def test_forward_backward_against_fp64(shape, x_dtype, act):
    S, K, N = shape
    inp = make_inputs(*shape)
    out, out2, z, (dx, dmu_w, dsg_w, dmu_b, dsg_b) = run_layer(inp, x_dtype, act)
    assert out.dtype == z.dtype == torch.bfloat16 and dx.dtype == x_dtype
    assert dmu_w.dtype == dsg_w.dtype == dmu_b.dtype == dsg_b.dtype == torch.float32
    assert torch.equal(out, out2)  # two applies, the same bits

    xb = inp["x"].bfloat16().double()
    w, b, e = ref_weight(inp)
    z_ref = xb @ w.T + b
    z_bound = E8 * z_ref.abs() + K * E23 * (xb.abs() @ w.abs().T)
    within(z, z_ref, z_bound, "Z")
    h_ref = act_ref(z_ref, act)[0]
    within(out, h_ref, E8 * h_ref.abs() + 1.1 * z_bound, "H")  # |act'| <= 1.1

    # backward from the stored Z; dZ = bf16(bf16(gw) * act'(Z))
    dz, slack = round_bf16(inp["gw"].bfloat16().double() * act_ref(z.detach().cpu().double(), act)[1])
    if act is None:
        assert not slack.any()
    bound_w = S * E23 * (dz.abs().T @ xb.abs()) + slack.T @ xb.abs()
    dw_ref = dz.T @ xb
    within(dmu_w, dw_ref, bound_w, "dmu_w")
    within(dsg_w, dw_ref * e, bound_w * e.abs(), "dsigma_w")
    bound_b = S * E23 * dz.abs().sum(0) + slack.sum(0)
    within(dmu_b, dz.sum(0), bound_b, "dmu_b")
    eo = inp["eps_out"].double()
    within(dsg_b, dz.sum(0) * eo, bound_b * eo.abs(), "dsigma_b")
    dx_ref = dz @ w
    within(dx, dx_ref, E8 * dx_ref.abs() + N * E23 * (dz.abs() @ w.abs()) + slack @ w.abs(), "dX")


@requires_gpu
@pytest.mark.parametrize("shape,act", [(SHAPES[0], "silu"), (SHAPES[1], "silu"), (SHAPES[4], "relu")])
def test_two_layer_chain_fused_act_backward(shape, act):
    """Layer 2's dgrad writes dZ1 = bf16(dX * act'(Z1)) itself: checked at the
    op, and through layer 1's gradients, whose reference takes the op's dZ1 as
    the operand the wgrad saw. The torso runs the same chain, forward and
    backward, bit for bit (it would not if it dropped the pre-activation)."""
    from stoix_amd import ops
    from stoix_amd.networks.torso import NoisyMLPTorso
    from stoix_amd.ops.noisy import ACT_CODES, noisy_linear_fused

    S, K, N = shape
    i1, i2 = make_inputs(S, K, 72), make_inputs(S, 72, N)
    l1, l2 = make_layer(i1), make_layer(i2)
    x = i1["x"].cuda()
    params = [l1.weight_mu, l1.weight_sigma, l1.bias_mu, l1.bias_sigma]
    gw = i2["gw"].cuda()
    with torch.autocast("cuda", torch.bfloat16):
        h1, pre = noisy_linear_fused(l1, x, act)
        out, _ = noisy_linear_fused(l2, h1, None, pre)
    g1 = torch.autograd.grad((out.float() * gw).sum(), params)
    z1 = pre[0].detach()

    torso = NoisyMLPTorso(K, (72, N), activation=act).cuda()
    torso.net = torso.net[:-1]
    torso.net[0], torso.net[2] = l1, l2
    with torch.autocast("cuda", torch.bfloat16):
        out_t = torso(x)
    gt = torch.autograd.grad((out_t.float() * gw).sum(), params)
    assert torch.equal(out_t, out) and all(torch.equal(a, b) for a, b in zip(gt, g1))

    dz2 = i2["gw"].bfloat16()
    dz1 = torch.full((S + 3, 72), 7.0, dtype=torch.bfloat16, device="cuda")
    assert ops.ext(required=True).noisy_linear_dgrad(
        dz2.cuda(), l2.weight_mu, l2.weight_sigma, l2.eps_in, l2.eps_out, z1, dz1[:S],
        ACT_CODES[act], True)
    assert (dz1[S:] == 7.0).all()  # rows past S keep the sentinel
    w2 = ref_weight(i2)[0]
    dact = act_ref(z1.cpu().double(), act)[1]
    dz1_ref = (dz2.double() @ w2) * dact
    within(dz1[:S], dz1_ref, E8 * dz1_ref.abs() + N * E23 * (dz2.double().abs() @ w2.abs()) * dact.abs(), "dZ1")

    dz1k = dz1[:S].cpu().double()  # what layer 1's wgrad was given
    xb, e1, eo1 = i1["x"].bfloat16().double(), ref_weight(i1)[2], i1["eps_out"].double()
    bound_w, bound_b = S * E23 * (dz1k.abs().T @ xb.abs()), S * E23 * dz1k.abs().sum(0)
    within(g1[0], dz1k.T @ xb, bound_w, "dmu_w1")
    within(g1[1], (dz1k.T @ xb) * e1, bound_w * e1.abs(), "dsigma_w1")
    within(g1[2], dz1k.sum(0), bound_b, "dmu_b1")
    within(g1[3], dz1k.sum(0) * eo1, bound_b * eo1.abs(), "dsigma_b1")


@requires_gpu
def test_noise_off_sentinel_and_repeatability():
    from stoix_amd import ops

    S, K, N = SHAPES[4]  # two wgrad slices
    inp = make_inputs(S, K, N)
    out, _, _, grads = run_layer(inp, torch.float32, None, noisy=False)
    assert grads[2] is None and grads[4] is None  # no sigma gradient without noise
    xb = inp["x"].bfloat16().double()
    w, b, _ = ref_weight(inp, noisy=False)
    z_ref = xb @ w.T + b
    within(out, z_ref, E8 * z_ref.abs() + K * E23 * (xb.abs() @ w.abs().T), "Z (mu only)")
    dz = inp["gw"].bfloat16().double()
    within(grads[1], dz.T @ xb, S * E23 * (dz.abs().T @ xb.abs()), "dmu_w (mu only)")
    within(grads[3], dz.sum(0), S * E23 * dz.abs().sum(0), "dmu_b (mu only)")
    dx_ref = dz @ w
    within(grads[0], dx_ref, E8 * dx_ref.abs() + N * E23 * (dz.abs() @ w.abs()), "dX (mu only)")

    again = run_layer(inp, torch.float32, "silu")
    first = run_layer(inp, torch.float32, "silu")
    assert torch.equal(first[0], again[0])
    assert all(torch.equal(a, b) for a, b in zip(first[3], again[3]))

    lin = make_layer(inp)
    pad = -(-(S + 5) * N // 8) * 8  # keeps the second row 16-byte aligned
    buf = torch.full((2, pad), -3.0, dtype=torch.bfloat16, device="cuda")
    z, h = buf[0, : S * N].view(S, N), buf[1, : S * N].view(S, N)
    assert ops.ext(required=True).noisy_linear_fwd(
        inp["x"].cuda(), lin.weight_mu, lin.weight_sigma, lin.bias_mu, lin.bias_sigma,
        lin.eps_in, lin.eps_out, z, h, 1, True)
    assert (buf[:, S * N:] == -3.0).all() and (z != -3.0).any() and (h != -3.0).any()

    gbuf = torch.full((4, N * K + 7), -3.0, device="cuda")  # wgrad outputs with a tail
    gw_, gb_ = gbuf[:2, : N * K], gbuf[2:, :N]
    assert ops.ext(required=True).noisy_linear_wgrad(
        inp["gw"].bfloat16().cuda(), inp["x"].cuda(), lin.eps_in, lin.eps_out,
        gw_[0].view(N, K), gw_[1].view(N, K), gb_[0], gb_[1])
    assert (gbuf[:2, N * K:] == -3.0).all() and (gbuf[2:, N:] == -3.0).all()


@requires_gpu
@pytest.mark.parametrize("knob", ["1", "0"])
def test_knob_routes_bank_and_torso(monkeypatch, knob):
    from stoix_amd.networks.layers import NoiseBank
    from stoix_amd.networks.torso import NoisyMLPTorso

    monkeypatch.setenv("STOIX_FUSED_NOISY", knob)
    torso = NoisyMLPTorso(40, (64, 51), activation="relu").cuda()
    bank = NoiseBank(torso)
    bank.resample()
    with torch.autocast("cuda", torch.bfloat16):
        y = torso(torch.randn(9, 40, device="cuda"))
    assert y.shape == (9, 51) and torch.isfinite(y).all()
    assert all((m._mat is None) == (knob == "1") for m in bank.layers)
    torso(torch.randn(9, 40, device="cuda"))  # fp32 compute: the torch path, whatever the knob
    assert all(m._mat is not None for m in bank.layers)


@requires_gpu
def test_noise_transform_bit_equal():
    from stoix_amd.ops.noisy import noise_transform_

    x = torch.randn(1031, generator=torch.Generator().manual_seed(3))
    x[:6] = torch.tensor([0.0, -0.0, 1e-40, -1e-40, 1.4e-45, -3e-39])
    x = x.cuda()
    ref = x.sign() * x.abs().sqrt()  # the sequence the kernel replaces
    got = noise_transform_(x.clone())
    assert torch.equal(got.view(torch.int32), ref.view(torch.int32))
    assert got[0].item() == 0.0 and got[2].item() > 0.0 > got[3].item()
