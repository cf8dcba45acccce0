"""GPU tests of the reverse-scan kernels (ops/csrc/scan.hip: GAE, lambda
returns, V-trace, retrace) against per-step float64 references, held to the
derived rounding bound ``k * EPS32 * A_t`` of tests/scan_oracle.py at every
element. tests/test_scan_bounds.py holds the float32 CPU branch of
ops/multistep.py to the same bounds on the same inputs."""
import pytest
import torch

import scan_oracle as so
from stoix_amd import ops
from stoix_amd.ops import multistep as ms

pytestmark = pytest.mark.gpu

DEV = "cuda"


@pytest.fixture(scope="module", autouse=True)
def ext():
    return ops.ext(required=True)


def _report():
    for key in sorted(so.RATIOS):
        if key.startswith("cuda:"):
            print(f"max error/bound {key} = {so.RATIOS[key]:.4f}")


@pytest.mark.parametrize("T,B", so.SHAPES, ids=lambda v: str(v))
def test_all_scans_within_rounding_bound(T, B):
    """B below one wave, the wave and block tails, several blocks; T = 1 and
    2; 10 % terminations and truncations, a step that is both, an
    all-truncated column; lambda in {0, 0.95, 1}; V-trace at the default
    clips and at clip_rho = 0.8, clip_pg_rho = 1.5, lambda = 0.9 with rho on
    the clips; all three V-trace outputs."""
    so.run_all(T, B, DEV, seed=1000 * T + B)
    _report()


def test_undamped_recursion():
    """d = 1 and lambda = 1: nothing damps the recursion, the magnitude grows
    with T and the bound grows with it."""
    x = so.make_inputs(37, 65, seed=7, undamped=True)
    so.check_gae(x, 1.0, DEV)
    so.check_lambda_returns(x, 1.0, DEV)
    so.check_vtrace(x, 1.0, 1.0, 1.0, DEV)
    so.check_retrace(x, 1.0, DEV)
    _report()


@pytest.mark.parametrize("T,B", [(37, 65), (5, 513)], ids=lambda v: str(v))
def test_transposed_views(T, B):
    """ff_mpo and ff_awr sample [B, T] windows and pass ``.transpose(0, 1)``
    views: same values, strides (1, T)."""
    x = so.make_inputs(T, B, seed=11)
    assert so.transposed("r", x["r"]).stride() == (1, T)
    so.check_gae(x, 0.95, DEV, view=so.transposed)
    so.check_lambda_returns(x, 0.95, DEV, view=so.transposed)
    so.check_vtrace(x, 0.9, 0.8, 1.5, DEV, view=so.transposed)
    so.check_offpolicy(x, DEV, view=so.transposed)
    so.check_retrace(x, 0.95, DEV, view=so.transposed)


def test_trailing_dimensions():
    """The documented [T, B, ...] contract: a [T, B, 3] input is the [T, 3 B]
    problem, and the outputs come back as [T, B, 3]."""
    T, B = 7, 43
    x = so.make_inputs(T, B * 3, seed=13)
    view = lambda key, t: t.reshape(T, B, 3)
    out = ms.batch_lambda_returns(x["r"].to(DEV).reshape(T, B, 3),
                                  x["d"].to(DEV).reshape(T, B, 3),
                                  x["v_t"].to(DEV).reshape(T, B, 3), 0.95)
    assert out.shape == (T, B, 3)
    flat = (T, B * 3)
    so.check_gae(x, 0.95, DEV, view=view, shape=flat)
    so.check_lambda_returns(x, 0.95, DEV, view=view, shape=flat)
    so.check_vtrace(x, 0.9, 0.8, 1.5, DEV, view=view, shape=flat)
    so.check_offpolicy(x, DEV, view=view, shape=flat)
    so.check_retrace(x, 0.95, DEV, view=view, shape=flat)


def test_broadcast_discount():
    """A [T, 1] discount broadcasts over the batch, as on the CPU branch."""
    T, B = 9, 130
    x = so.make_inputs(T, B, seed=17)
    x["d"] = x["d"][:, :1].expand(T, B).contiguous()  # what the oracle sees
    view = lambda key, t: t[:, :1].contiguous() if key == "d" else t
    so.check_gae(x, 0.95, DEV, view=view)
    so.check_lambda_returns(x, 0.95, DEV, view=view)
    so.check_vtrace(x, 0.9, 0.8, 1.5, DEV, view=view)
    so.check_offpolicy(x, DEV, view=view)


# --------------------------------------------------- the bindings themselves
def _binding_calls(ext, x, out_a, out_b):
    """name -> (operands in binding order, call). ``trunc`` is uint8."""
    lam = 0.95
    return {
        "gae": (["r", "d", "v_tm1", "v_t", "trunc"],
                lambda a: ext.gae(a["r"], a["d"], a["v_tm1"], a["v_t"], a["trunc"],
                                  out_a, out_b, lam)),
        "lambda_returns": (["r", "d", "v_t"],
                           lambda a: ext.lambda_returns(a["r"], a["d"], a["v_t"], out_a, lam)),
        "vtrace": (["v_tm1", "v_t", "r", "d", "rho"],
                   lambda a: ext.vtrace(a["v_tm1"], a["v_t"], a["r"], a["d"], a["rho"],
                                        out_a, out_b, lam, 0.8, 1.5)),
        "offpolicy_returns": (["q", "v_t", "r", "d", "c"],
                              lambda a: ext.offpolicy_returns(a["q"], a["v_t"], a["r"], a["d"],
                                                              a["c"], out_a)),
    }


def _device_inputs(T, B, seed):
    x = so.make_inputs(T, B, seed)
    x["trunc"] = x["trunc"].to(torch.uint8)
    return {k: v.to(DEV) for k, v in x.items()}


@pytest.mark.parametrize("T,B", [(1, 1), (2, 63), (37, 65), (37, 513)], ids=lambda v: str(v))
def test_bindings_write_every_element_and_nothing_else(ext, T, B):
    """Outputs are the first T rows of a NaN-filled [T + 1, B] buffer: rows
    < T come back finite everywhere, row T stays NaN."""
    x = _device_inputs(T, B, seed=19)
    for name in ("gae", "lambda_returns", "vtrace", "offpolicy_returns"):
        buf_a = torch.full((T + 1, B), float("nan"), device=DEV)
        buf_b = torch.full((T + 1, B), float("nan"), device=DEV)
        operands, call = _binding_calls(ext, x, buf_a[:T], buf_b[:T])[name]
        call(x)
        two_outputs = name in ("gae", "vtrace")
        for buf in (buf_a, buf_b) if two_outputs else (buf_a,):
            assert torch.isfinite(buf[:T]).all(), f"{name}: unwritten output elements"
            assert torch.isnan(buf[T]).all(), f"{name}: wrote past row T"
        if not two_outputs:
            assert torch.isnan(buf_b).all()


def test_bindings_refuse_mismatched_operands(ext):
    """Every operand is checked on the host before anything is launched: a
    wrong shape, dtype, layout or device raises."""
    T, B = 4, 33
    x = _device_inputs(T, B, seed=23)
    out_a = torch.zeros(T, B, device=DEV)
    out_b = torch.zeros(T, B, device=DEV)
    calls = _binding_calls(ext, x, out_a, out_b)
    # First an operand that is too LARGE, which no kernel can overrun: should
    # the checks ever be missing, the test stops here, before any call whose
    # operand is too small.
    with pytest.raises(RuntimeError):
        ext.lambda_returns(x["r"], torch.cat([x["d"], x["d"]], 1), x["v_t"], out_a, 0.95)
    for name, (operands, call) in calls.items():
        call(x)  # the well-formed call is accepted
        for key in operands:
            good = x[key]
            bad = {
                "column": good[:, :1].contiguous(),
                "one row short": good[: T - 1].contiguous(),
                "one column more": torch.cat([good, good[:, :1]], 1),
                "flattened": good.reshape(-1),
                "strided": torch.cat([good, good], 1)[:, ::2],
                "float64": good.double(),
                "cpu": good.cpu(),
            }
            # (r_t defines the shape: with a wrong r_t the other operands mismatch)
            for why, t in bad.items():
                with pytest.raises(RuntimeError):
                    call({**x, key: t})
    # outputs are checked like the inputs
    short = torch.zeros(T - 1, B, device=DEV)
    with pytest.raises(RuntimeError):
        ext.lambda_returns(x["r"], x["d"], x["v_t"], short, 0.95)
    with pytest.raises(RuntimeError):
        ext.gae(x["r"], x["d"], x["v_tm1"], x["v_t"], x["trunc"], out_a, short, 0.95)
    with pytest.raises(RuntimeError):
        ext.vtrace(x["v_tm1"], x["v_t"], x["r"], x["d"], x["rho"], short, out_b, 0.95, 1.0, 1.0)
    with pytest.raises(RuntimeError):
        ext.offpolicy_returns(x["q"], x["v_t"], x["r"], x["d"], x["c"], short)
    # an empty trunc_t means "no truncation" and is accepted
    ext.gae(x["r"], x["d"], x["v_tm1"], x["v_t"],
            torch.empty(0, dtype=torch.uint8, device=DEV), out_a, out_b, 0.95)
    torch.cuda.synchronize()
