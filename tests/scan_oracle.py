"""fp64 oracles, inputs and rounding bounds for the reverse-scan estimators
(GAE, lambda returns, V-trace, retrace), shared by the GPU tests of
ops/csrc/scan.hip (tests/test_scan_gpu.py) and the CPU check that the float32
torch branch of ops/multistep.py meets the same bounds
(tests/test_scan_bounds.py).

Every reference is a per-step float64 loop over ``[T, B]`` tensors written
from the recursion in the estimator's docstring. It takes the float32-rounded
``lambda_`` and clip thresholds, which is what the kernels receive, so the
only difference left to bound is float32 rounding inside the scan.

The bound
---------
Each recursion has the form ``x_t = sum_i term_i + coef_t * x_{t+1}``. Let
``A_t`` be the same recursion run on absolute values in float64 (the running
magnitude). A float32 evaluation rounds each term at most K times on its way
into ``x_t`` (K = the longest chain of roundings in one step, counted from
scan.hip below), each rounding being a relative perturbation of at most
u = 2**-24. To first order the error obeys

    e_t <= K u sum_i |term_i| + |coef_t| (K u |x_{t+1}| + e_{t+1})

so by induction ``e_t <= K u A_t``: the error carried in from step t+1 is
already inside ``|coef_t| A_{t+1}``. Terms of order u**2 are below 1e-6 of
that. The asserted bound is ``k * EPS32 * A_t`` with ``k = K + 1`` and
``EPS32 = 2**-23 = 2 u``. Contracting ``a * b + c`` into an FMA removes a
rounding and never adds one, so the count holds for any contraction.
"""
from __future__ import annotations

from typing import Dict

import numpy as np
import torch

from stoix_amd.ops import multistep as ms

EPS32 = float(torch.finfo(torch.float32).eps)  # 2**-23

SHAPES = [(T, B) for T in (1, 2, 37) for B in (1, 63, 65, 257, 513)]
LAMBDAS = (0.0, 0.95, 1.0)

# Roundings on the longest chain of one step, from scan.hip (k = K + 1):
#   gae_kernel, adv:      d*v_t, +r, -v_tm1, delta + (...)              K = 4
#                         [d*lambda, *acc, +delta is 3; *cont is exact]
#   gae_kernel, target:   adv, then acc + v_tm1                         K = 5
#   lambda_returns:       1-lambda, *v_t, + lambda*acc, d*(...), r +    K = 5
#   vtrace, errors:       d*v_t, +r, -v_tm1, rho_c*(...), delta + (...) K = 5
#                         [lambda*min(rho,1), d*c, *acc, +delta is 4]
#   vtrace, pg_adv:       errors (5), +v_tm1, d*vs, r+, -v_tm1, pg_rho* K = 10
#   vtrace, q_estimate:   errors (5), +v_tm1, d*vs, r+                  K = 8
#   offpolicy_returns:    c*q, v - (...), + c*g, d*(...), r +           K = 5
#   retrace c_t = lambda * min(exp(log_rho), 1): expf is within 1 ulp
#   (2 u) and the product rounds once, 3 more on every term holding c   K = 8
K_GAE_ADV = 4 + 1
K_GAE_TARGET = 5 + 1
K_LAMBDA = 5 + 1
K_VTRACE_ERR = 5 + 1
K_VTRACE_PG = 10 + 1
K_VTRACE_Q = 8 + 1
K_OFFPOLICY = 5 + 1
K_RETRACE = 8 + 1

#: largest error / bound seen per (device, quantity); the tests print it
RATIOS: Dict[str, float] = {}


def f32(x: float) -> float:
    """The float32 rounding of a Python float, as a Python float."""
    return float(np.float32(x))


def make_inputs(T: int, B: int, seed: int, undamped: bool = False) -> Dict[str, torch.Tensor]:
    """Float32 CPU inputs ``[T, B]``. Discounts are 0.99 with ~10 % exact
    zeros (terminations); ~10 % of steps are truncated; step (0, 0) is both
    terminated and truncated; the last column is truncated at every step.
    ``rho`` is log-normal around 1 with entries exactly on the clips 0.8, 1
    and 1.5; ``log_rho`` has both signs. ``undamped`` gives d = 1 everywhere
    and no truncation."""
    g = torch.Generator().manual_seed(seed)
    rn = lambda: torch.randn(T, B, generator=g)
    x = {"r": rn(), "v_tm1": rn(), "v_t": rn(), "q": rn()}
    if undamped:
        x["d"] = torch.ones(T, B)
        x["trunc"] = torch.zeros(T, B, dtype=torch.bool)
    else:
        x["d"] = (torch.rand(T, B, generator=g) > 0.1).float() * 0.99
        x["trunc"] = torch.rand(T, B, generator=g) < 0.1
        x["d"][0, 0] = 0.0
        x["trunc"][0, 0] = True
        x["trunc"][:, -1] = True
    rho = (0.5 * rn()).exp()
    flat = rho.view(-1)
    flat[0::7] = f32(0.8)
    flat[3::11] = 1.0
    flat[5::13] = 1.5
    x["rho"] = rho
    x["log_rho"] = 0.5 * rn()
    x["c"] = torch.rand(T, B, generator=g)
    return x


def _d(t: torch.Tensor) -> torch.Tensor:
    return t.detach().cpu().double()


# ------------------------------------------------------------ fp64 references
def ref_gae(r, d, v_tm1, v_t, trunc, lam):
    r, d, v_tm1, v_t = map(_d, (r, d, v_tm1, v_t))
    cont = 1.0 - _d(trunc)
    T = r.shape[0]
    adv, A = torch.empty_like(r), torch.empty_like(r)
    acc, a = torch.zeros_like(r[0]), torch.zeros_like(r[0])
    for t in range(T - 1, -1, -1):
        coef = d[t] * lam * cont[t]
        acc = r[t] + d[t] * v_t[t] - v_tm1[t] + coef * acc
        a = r[t].abs() + (d[t] * v_t[t]).abs() + v_tm1[t].abs() + coef.abs() * a
        adv[t], A[t] = acc, a
    return {"adv": adv, "A_adv": A, "target": adv + v_tm1, "A_target": A + v_tm1.abs()}


def ref_lambda_returns(r, d, v_t, lam):
    r, d, v_t = map(_d, (r, d, v_t))
    T = r.shape[0]
    out, A = torch.empty_like(r), torch.empty_like(r)
    acc, a = v_t[T - 1].clone(), v_t[T - 1].abs()
    for t in range(T - 1, -1, -1):
        acc = r[t] + d[t] * ((1.0 - lam) * v_t[t] + lam * acc)
        a = r[t].abs() + d[t].abs() * ((1.0 - lam) * v_t[t].abs() + lam * a)
        out[t], A[t] = acc, a
    return {"out": out, "A": A}


def ref_vtrace(v_tm1, v_t, r, d, rho, lam, clip_rho, clip_pg_rho):
    v_tm1, v_t, r, d, rho = map(_d, (v_tm1, v_t, r, d, rho))
    T = r.shape[0]
    rho_c = rho.clamp(max=clip_rho)
    c = lam * rho.clamp(max=1.0)
    err, A = torch.empty_like(r), torch.empty_like(r)
    acc, a = torch.zeros_like(r[0]), torch.zeros_like(r[0])
    for t in range(T - 1, -1, -1):
        acc = rho_c[t] * (r[t] + d[t] * v_t[t] - v_tm1[t]) + d[t] * c[t] * acc
        a = rho_c[t] * (r[t].abs() + (d[t] * v_t[t]).abs() + v_tm1[t].abs()) \
            + (d[t] * c[t]).abs() * a
        err[t], A[t] = acc, a
    # vs_{t+1}, bootstrapped from v_t at the end, and its magnitude
    vs_next = torch.cat([err[1:] + v_tm1[1:], v_t[-1:]], 0)
    A_vs = torch.cat([A[1:] + v_tm1[1:].abs(), v_t[-1:].abs()], 0)
    q = r + d * vs_next
    A_q = r.abs() + d.abs() * A_vs
    pg_rho = rho.clamp(max=clip_pg_rho)
    return {"errors": err, "A_errors": A, "q": q, "A_q": A_q,
            "pg": pg_rho * (q - v_tm1), "A_pg": pg_rho * (A_q + v_tm1.abs())}


def ref_offpolicy(q, v_t, r, d, c):
    q, v_t, r, d, c = map(_d, (q, v_t, r, d, c))
    T = r.shape[0]
    out, A = torch.empty_like(r), torch.empty_like(r)
    g = r[T - 1] + d[T - 1] * v_t[T - 1]
    a = r[T - 1].abs() + (d[T - 1] * v_t[T - 1]).abs()
    out[T - 1], A[T - 1] = g, a
    for t in range(T - 2, -1, -1):
        g = r[t] + d[t] * (v_t[t] - c[t] * q[t] + c[t] * g)
        a = r[t].abs() + d[t].abs() * (v_t[t].abs() + (c[t] * q[t]).abs() + c[t].abs() * a)
        out[t], A[t] = g, a
    return {"out": out, "A": A}


# ------------------------------------------------------------------ assertion
def assert_within(name: str, got: torch.Tensor, ref: torch.Tensor, A: torch.Tensor,
                  k: int) -> float:
    """``|got - ref| <= k * EPS32 * A`` at every element, none masked out.
    Records and returns the largest error / bound."""
    assert got.shape == ref.shape, f"{name}: shape {tuple(got.shape)} vs {tuple(ref.shape)}"
    got64 = _d(got)
    assert torch.isfinite(got64).all(), f"{name}: non-finite output"
    err = (got64 - ref).abs()
    bound = k * EPS32 * A
    # where the magnitude is 0 every term is 0 and the result is exactly 0
    ratio = torch.where(bound > 0, err / bound.clamp(min=1e-300),
                        torch.where(err > 0, torch.full_like(err, float("inf")),
                                    torch.zeros_like(err)))
    worst = float(ratio.max())
    key = f"{got.device.type}:{name}"
    RATIOS[key] = max(RATIOS.get(key, 0.0), worst)
    assert worst <= 1.0, f"{name}: error / bound = {worst:.3f} (k = {k})"
    return worst


# -------------------------------------- one call of each estimator vs its oracle
def check_gae(x, lam, device, view=lambda key, t: t, shape=None):
    """``view(key, tensor)`` maps each reference-layout input, already on
    ``device``, to what is handed to multistep; ``shape`` reshapes the
    outputs back to the reference layout."""
    lam32 = f32(lam)
    ref = ref_gae(x["r"], x["d"], x["v_tm1"], x["v_t"], x["trunc"], lam32)
    a = {k: view(k, x[k].to(device)) for k in ("r", "d", "v_tm1", "v_t", "trunc")}
    adv, tgt = ms.batch_truncated_generalized_advantage_estimation(
        a["r"], a["d"], lam, a["v_tm1"], a["v_t"], truncation_t=a["trunc"])
    if shape is not None:
        adv, tgt = adv.reshape(shape), tgt.reshape(shape)
    assert_within("gae.adv", adv, ref["adv"], ref["A_adv"], K_GAE_ADV)
    assert_within("gae.target", tgt, ref["target"], ref["A_target"], K_GAE_TARGET)


def check_lambda_returns(x, lam, device, view=lambda key, t: t, shape=None):
    ref = ref_lambda_returns(x["r"], x["d"], x["v_t"], f32(lam))
    a = {k: view(k, x[k].to(device)) for k in ("r", "d", "v_t")}
    out = ms.batch_lambda_returns(a["r"], a["d"], a["v_t"], lam)
    if shape is not None:
        out = out.reshape(shape)
    assert_within("lambda_returns", out, ref["out"], ref["A"], K_LAMBDA)


def check_vtrace(x, lam, clip_rho, clip_pg_rho, device, view=lambda key, t: t, shape=None):
    ref = ref_vtrace(x["v_tm1"], x["v_t"], x["r"], x["d"], x["rho"], f32(lam),
                     f32(clip_rho), f32(clip_pg_rho))
    a = {k: view(k, x[k].to(device)) for k in ("v_tm1", "v_t", "r", "d", "rho")}
    err, pg, q = ms.vtrace_td_error_and_advantage(
        a["v_tm1"], a["v_t"], a["r"], a["d"], a["rho"], lambda_=lam,
        clip_rho_threshold=clip_rho, clip_pg_rho_threshold=clip_pg_rho)
    if shape is not None:
        err, pg, q = err.reshape(shape), pg.reshape(shape), q.reshape(shape)
    assert_within("vtrace.errors", err, ref["errors"], ref["A_errors"], K_VTRACE_ERR)
    assert_within("vtrace.pg_advantage", pg, ref["pg"], ref["A_pg"], K_VTRACE_PG)
    assert_within("vtrace.q_estimate", q, ref["q"], ref["A_q"], K_VTRACE_Q)


def check_offpolicy(x, device, view=lambda key, t: t, shape=None):
    ref = ref_offpolicy(x["q"], x["v_t"], x["r"], x["d"], x["c"])
    a = {k: view(k, x[k].to(device)) for k in ("q", "v_t", "r", "d", "c")}
    out = ms.batch_general_off_policy_returns_from_q_and_v(
        a["q"], a["v_t"], a["r"], a["d"], a["c"])
    if shape is not None:
        out = out.reshape(shape)
    assert_within("offpolicy_returns", out, ref["out"], ref["A"], K_OFFPOLICY)


def check_retrace(x, lam, device, view=lambda key, t: t, shape=None):
    """Through ``batch_retrace_continuous``: c_t = lambda * min(exp(log_rho), 1)
    is formed in float32 by torch, in float64 here."""
    c64 = f32(lam) * _d(x["log_rho"]).exp().clamp(max=1.0)
    ref = ref_offpolicy(x["q"], x["v_t"], x["r"], x["d"], c64)
    a = {k: view(k, x[k].to(device)) for k in ("q", "v_t", "r", "d", "log_rho")}
    out = ms.batch_retrace_continuous(a["q"], a["q"], a["v_t"], a["r"], a["d"],
                                      a["log_rho"], lam)
    if shape is not None:
        out = out.reshape(shape)
    assert_within("retrace", out, ref["out"], ref["A"], K_RETRACE)


def transposed(key: str, t: torch.Tensor) -> torch.Tensor:
    """The ``[T, B]`` view of a contiguous ``[B, T]`` tensor holding the same
    values: what ff_mpo and ff_awr pass after sampling ``[B, T]`` windows."""
    return t.transpose(0, 1).contiguous().transpose(0, 1)


def run_all(T: int, B: int, device: str, seed: int = 0) -> None:
    """Every estimator on one shape, for every lambda."""
    x = make_inputs(T, B, seed)
    for lam in LAMBDAS:
        check_gae(x, lam, device)
        check_lambda_returns(x, lam, device)
        check_retrace(x, lam, device)
        check_vtrace(x, lam, 1.0, 1.0, device)
    check_vtrace(x, 0.9, 0.8, 1.5, device)
    check_offpolicy(x, device)
