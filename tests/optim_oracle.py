"""float64 oracle, cases and rounding bounds for the fused clip + Adam kernels
(ops/csrc/optim.hip: ``fused_adam`` and ``fused_adam_bf16``), shared by
tests/test_optim_gpu.py (the kernels) and tests/test_optim_bounds.py (the same
formula evaluated in float32 torch on the CPU, which must meet the same
bounds, or the bounds are wrong).

The reference is clip-by-global-norm + one Adam step written out in float64
on the float32-rounded hyper-parameters, with the project's clip rule:

    norm  = sqrt(sum(grad ** 2)) * grad_scale
    clip  = grad_scale * max_norm / (norm + 1e-6)   if max_norm > 0 and norm > max_norm
            grad_scale                              otherwise
    g     = grad * clip
    m     = b1 m + (1 - b1) g          v = b2 v + (1 - b2) g g
    param = param - lr (m / (1 - b1 ** t)) / (sqrt(v / (1 - b2 ** t)) + eps)

Bounds
------
Every float32 operation is a relative perturbation of at most u = 2**-24.
The bounds below are first order in u and are written with EPS32 = 2 u per
rounding, which leaves a factor of two for the higher-order terms; the one
exception is the last rounding of ``param`` itself, taken at u exactly.

* ``sqnorm[0]``: all terms are non-negative, so a sum is off by at most
  (longest chain of additions) * u relative. The chain is the per-thread
  trips (8 additions per 16-byte vector of bf16, whose squares are exact in
  float32; for float32 gradients one addition per vector plus 4 for the
  rounded squares and the three additions inside the vector), one or two
  more for the tail, 6 shuffle steps, 4 waves, and the blocks: ``blocks``
  atomic additions in any order, or ceil(blocks / 64) + 6 in the ordered
  form. ``rho_sq = chain * EPS32``.
* ``clip``: sqrt halves rho_sq and rounds; then * grad_scale, + 1e-6,
  grad_scale * max_norm and the division: ``rho_clip = (chain / 2 + 5) *
  EPS32`` when clipped, 0 otherwise. ``g`` rounds once more.
* ``m``: 1 - b1, * g, b1 * m, + : the old term is rounded twice, the new one
  three times, and the new one carries rho_g. ``v`` likewise with g twice.
* bias correction: powf is within 1 ulp (2 u) of b ** t and 1 - b ** t
  rounds once; the cancellation amplifies the first by b**t / (1 - b**t):
  ``rho_bc = EPS32 * (1 + 2 b**t / (1 - b**t))``.
* the update lr * (m / bc1) / (sqrt(v / bc2) + eps): two divisions, the
  square root (which halves what it is given), + eps, lr * and / : see
  ``reference``. The applied update ``param_after - param_before`` adds the
  final rounding of param, u * |param_after|.
"""
from __future__ import annotations

import math
from dataclasses import dataclass
from typing import Dict

import numpy as np
import torch

EPS32 = float(torch.finfo(torch.float32).eps)  # 2**-23
U32 = EPS32 / 2

LR, B1, B2, EPS = 3e-4, 0.9, 0.999, 1e-8
THREADS, MAX_BLOCKS = 256, 2048  # the launchers' block size and grid cap
ORDERED_LEN = 1 + MAX_BLOCKS  # sqnorm buffer with room for one partial per block
SENTINEL = 7.0  # what the test leaves in sqnorm where the kernels must not write

WRAP_UPDATE = MAX_BLOCKS * THREADS + 13  # the update kernel's stride loop wraps
NORM_BF16 = MAX_BLOCKS * THREADS * 8 + 3  # every bf16 norm thread busy, plus a tail
WRAP_NORM_BF16 = MAX_BLOCKS * THREADS * 8 + 11  # one vector more: thread 0 takes a 2nd trip
WRAP_NORM_F32 = MAX_BLOCKS * THREADS * 4 + 5  # the fp32 norm kernel wraps
SMALL_SIZES = (1, 7, 8, 9, 1023, 100_003)

RATIOS: Dict[str, float] = {}


def f32(x: float) -> float:
    return float(np.float32(x))


@dataclass(frozen=True)
class Case:
    n: int
    kind: str = "bf16"  # "bf16": fused_adam_bf16, "f32": fused_adam
    clip: str = "active"  # "off" (max_norm = 0), "inactive" (norm < max_norm), "active"
    grad_scale: float = 1.0
    do_prologue: int = 1
    sqnorm_len: int = 1  # 1: atomic norm, ORDERED_LEN: ordered norm
    mirror: bool = True  # False: param_bf16 is empty
    step0: int = 0
    zero_grad: bool = False
    seed: int = 0

    @property
    def id(self) -> str:
        s = f"{self.kind}-n{self.n}-{self.clip}-gs{self.grad_scale:g}-pro{self.do_prologue}"
        s += f"-sq{self.sqnorm_len}-t{self.step0}"
        return s + ("" if self.mirror else "-nomirror") + ("-zerograd" if self.zero_grad else "")


def norm_launch(n: int, vec: int):
    """(blocks, vector trips of the busiest thread) of the norm kernel, as
    launch_fused_adam{,_bf16} size it; vec = elements per 16-byte load."""
    nvec = n // vec
    blocks = min(max((nvec + THREADS - 1) // THREADS, 1), MAX_BLOCKS)
    return blocks, -(-nvec // (blocks * THREADS))


def sqnorm_chain(case: Case) -> int:
    vec = 8 if case.kind == "bf16" else 4
    blocks, trips = norm_launch(case.n, vec)
    tail = 1 if case.n % vec else 0
    per_thread = 8 * trips + tail if vec == 8 else trips + 4 + 2 * tail
    across = -(-blocks // 64) + 6 if case.sqnorm_len >= 1 + blocks else blocks
    return per_thread + 6 + 4 + across


def make_inputs(case: Case) -> Dict[str, torch.Tensor]:
    """CPU inputs. ``max_norm`` is placed a factor of 2 above ("inactive") or
    at 0.37 of ("active") the float64 norm of grad * grad_scale, far from
    the branch relative to any rounding."""
    g = torch.Generator().manual_seed(case.seed * 7919 + case.n % 1000)
    n = case.n
    x = {"p": torch.randn(n, generator=g)}
    if case.zero_grad:
        x["g"] = torch.zeros(n)
        x["m"] = torch.zeros(n)
        x["v"] = torch.zeros(n)
    else:
        x["g"] = torch.randn(n, generator=g) * 0.01
        x["m"] = torch.randn(n, generator=g) * 0.01
        x["v"] = torch.rand(n, generator=g) * 1e-4
    if case.kind == "bf16":
        x["g"] = x["g"].bfloat16()
    norm = math.sqrt(float((x["g"].double() ** 2).sum())) * f32(case.grad_scale)
    if case.clip == "off":
        x["max_norm"] = 0.0
    elif case.zero_grad:
        x["max_norm"] = 0.5
    else:
        x["max_norm"] = norm * (2.0 if case.clip == "inactive" else 0.37)
    return x


def reference(case: Case, x: Dict[str, torch.Tensor]) -> Dict[str, torch.Tensor]:
    """float64 result and the bound on every asserted quantity."""
    p0, g, m0, v0 = (x[k].double() for k in ("p", "g", "m", "v"))
    lr, b1, b2, eps, mn, gs = (f32(a) for a in (LR, B1, B2, EPS, x["max_norm"], case.grad_scale))
    chain = sqnorm_chain(case)
    sq = float((g * g).sum())
    norm = math.sqrt(sq) * gs
    clipped = mn > 0 and norm > mn
    assert clipped == (case.clip == "active" and not case.zero_grad)
    clip = gs * mn / (norm + f32(1e-6)) if clipped else gs
    rho_clip = (chain / 2 + 5) * EPS32 if clipped else 0.0
    rho_g = rho_clip + EPS32

    t = case.step0 + 1
    pw1, pw2 = b1 ** t, b2 ** t
    bc1, bc2 = 1.0 - pw1, 1.0 - pw2
    rho_bc1 = EPS32 * (1 + 2 * pw1 / bc1)
    rho_bc2 = EPS32 * (1 + 2 * pw2 / bc2)

    gg = g * clip
    new_m = (1.0 - b1) * gg
    new_v = (1.0 - b2) * gg * gg
    m = b1 * m0 + new_m
    v = b2 * v0 + new_v
    E_m = EPS32 * (2 * (b1 * m0).abs() + 3 * new_m.abs()) + rho_g * new_m.abs()
    E_v = EPS32 * (2 * b2 * v0 + 4 * new_v) + 2 * rho_g * new_v

    mhat, vhat = m / bc1, v / bc2
    E_mhat = E_m / bc1 + mhat.abs() * (rho_bc1 + EPS32)
    E_vhat = E_v / bc2 + vhat * (rho_bc2 + EPS32)
    s = vhat.sqrt()
    E_s = torch.where(s > 0, E_vhat / (2 * s).clamp(min=1e-300), torch.zeros_like(s)) + EPS32 * s
    den = s + eps
    E_den = E_s + EPS32 * den
    upd = lr * mhat / den
    E_upd = lr * E_mhat / den + upd.abs() * (E_den / den + 2 * EPS32)
    p = p0 - upd
    return {
        "sq": sq, "chain": chain, "step": t,
        "m": m, "E_m": E_m, "v": v, "E_v": E_v,
        "delta": -upd, "E_delta": E_upd + U32 * (p.abs() + E_upd),
    }


def torch32_step(case: Case, x: Dict[str, torch.Tensor]) -> Dict[str, torch.Tensor]:
    """The kernels' formula, operation by operation, in float32 torch on the
    CPU. Returns what ``run`` in the GPU tests returns."""
    F = lambda a: torch.tensor(a, dtype=torch.float32)
    lr, b1, b2, eps, mn, gs = (F(a) for a in (LR, B1, B2, EPS, x["max_norm"], case.grad_scale))
    g, p, m, v = x["g"].float(), x["p"].clone(), x["m"].clone(), x["v"].clone()
    sqnorm = torch.full((case.sqnorm_len,), SENTINEL)
    sqnorm[0] = 0.0
    clip = gs.clone()
    if float(mn) > 0:
        sqnorm[0] = (g * g).sum()
        norm = sqnorm[0].sqrt() * gs
        if float(norm) > float(mn):
            clip = gs * mn / (norm + F(1e-6))
    t = case.step0 + 1
    bc1 = 1.0 - torch.pow(b1, F(float(t)))
    bc2 = 1.0 - torch.pow(b2, F(float(t)))
    gg = g * clip
    m = b1 * m + (1.0 - b1) * gg
    v = b2 * v + (1.0 - b2) * gg * gg
    p = p - lr * (m / bc1) / ((v / bc2).sqrt() + eps)
    return {"p": p, "m": m, "v": v, "step": torch.tensor([t]), "sqnorm": sqnorm,
            "p16": p.bfloat16() if case.mirror and case.kind == "bf16" else None}


def _ratio(name: str, err: torch.Tensor, bound: torch.Tensor) -> float:
    """Largest err / bound; where the bound is 0 the value must be exact."""
    assert not ((bound <= 0) & (err > 0)).any(), f"{name}: inexact where the result is exact"
    r = float((err / bound.clamp(min=1e-300)).max()) if err.numel() else 0.0
    RATIOS[name] = max(RATIOS.get(name, 0.0), r)
    return r


def check(case: Case, x: Dict[str, torch.Tensor], got: Dict[str, torch.Tensor], who: str) -> None:
    """Assert everything the issue lists after one call. ``who`` tags the
    recorded ratios ("hip" or "torch32")."""
    ref = reference(case, x)
    tag = f"{who}:{case.kind}"
    assert got["step"].tolist() == [ref["step"]], f"{case.id}: step_t"

    for key in ("m", "v"):
        err = (got[key].double() - ref[key]).abs()
        r = _ratio(f"{tag}:exp_avg{'_sq' if key == 'v' else ''}", err, ref["E_" + key])
        assert r <= 1.0, f"{case.id}: {key} error / bound = {r:.3f}"

    delta = got["p"].double() - x["p"].double()
    r = _ratio(f"{tag}:update", (delta - ref["delta"]).abs(), ref["E_delta"])
    assert r <= 1.0, f"{case.id}: applied update error / bound = {r:.3f}"
    if case.zero_grad:
        assert torch.equal(got["p"], x["p"]), f"{case.id}: a zero gradient moved param"
        assert not got["m"].any() and not got["v"].any()

    sqnorm = got["sqnorm"]
    assert sqnorm.numel() == case.sqnorm_len
    if case.clip == "off":
        # the norm kernel is not launched: 0 from the prologue, nothing else
        assert float(sqnorm[0]) == 0.0, f"{case.id}: sqnorm[0] = {float(sqnorm[0])}"
        assert (sqnorm[1:] == SENTINEL).all(), f"{case.id}: sqnorm written without a norm pass"
    else:
        err = torch.tensor([abs(float(sqnorm[0]) - ref["sq"])], dtype=torch.float64)
        bound = torch.tensor([ref["chain"] * EPS32 * ref["sq"]], dtype=torch.float64)
        r = _ratio(f"{tag}:sqnorm", err, bound)
        assert r <= 1.0, f"{case.id}: sqnorm error / bound = {r:.3f} (chain {ref['chain']})"
        if who == "hip" and case.sqnorm_len > 1:
            blocks, _ = norm_launch(case.n, 8)
            assert (sqnorm[1 + blocks:] == SENTINEL).all(), f"{case.id}: wrote past the partials"
            assert (sqnorm[1: 1 + blocks] != SENTINEL).all(), f"{case.id}: a partial is missing"

    if case.kind == "bf16" and case.mirror:
        # the mirror is one round-to-nearest-even of the float32 master
        assert torch.equal(got["p16"], got["p"].bfloat16()), f"{case.id}: bf16 mirror"


# ------------------------------------------------------------------ the cases
def _cases():
    out = []
    # every size in every clip state; the norm alternates atomic / ordered
    sizes = SMALL_SIZES + (WRAP_UPDATE, NORM_BF16, WRAP_NORM_BF16)
    for i, n in enumerate(sizes):
        for j, clip in enumerate(("off", "inactive", "active")):
            out.append(Case(n, clip=clip, sqnorm_len=ORDERED_LEN if (i + j) % 2 else 1, seed=1))
    # grad_scale x clip state x prologue x norm form, mirror on and off
    for n in (1023, 100_003):
        k = 0
        for gs in (1.0, 0.125):
            for clip in ("inactive", "active"):
                for pro in (0, 1):
                    for sq in (1, ORDERED_LEN):
                        out.append(Case(n, clip=clip, grad_scale=gs, do_prologue=pro,
                                        sqnorm_len=sq, mirror=bool(k % 2), seed=2))
                        k += 1
    out.append(Case(1023, clip="off", grad_scale=0.125, do_prologue=0, sqnorm_len=ORDERED_LEN,
                    mirror=False, seed=2))
    for clip in ("off", "active"):
        for sq in (1, ORDERED_LEN):
            out.append(Case(1023, clip=clip, sqnorm_len=sq, zero_grad=True, seed=3))
    for step0 in (0, 9, 999, 10 ** 6):
        for gs in (1.0, 0.125):
            out.append(Case(1023, step0=step0, grad_scale=gs, sqnorm_len=ORDERED_LEN, seed=4))
    # fused_adam (float32 gradients) at the same sizes
    for n in SMALL_SIZES + (WRAP_UPDATE, WRAP_NORM_F32):
        for clip in ("off", "inactive", "active"):
            out.append(Case(n, kind="f32", clip=clip, seed=5))
    out.append(Case(1023, kind="f32", clip="active", zero_grad=True, seed=5))
    for step0 in (9, 999, 10 ** 6):
        out.append(Case(1023, kind="f32", step0=step0, seed=6))
    return out


CASES = _cases()
