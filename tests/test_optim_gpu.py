"""GPU tests of the fused clip + Adam kernels (ops/csrc/optim.hip:
``fused_adam_bf16`` with its bf16 mirror, and ``fused_adam``) against the
float64 reference of tests/optim_oracle.py: step_t exactly, exp_avg,
exp_avg_sq, the applied update and sqnorm[0] within derived rounding bounds,
and the mirror bit-equal to one rounding of the float32 master.
tests/test_optim_bounds.py holds the same formula in float32 torch to the
same bounds on the CPU."""
import pytest
import torch

import optim_oracle as oo
from stoix_amd import ops

pytestmark = pytest.mark.gpu

DEV = "cuda"


@pytest.fixture(scope="module", autouse=True)
def ext():
    return ops.ext(required=True)


def run(ext, case, x):
    """One call of the kernel under test; everything it may write, on the CPU."""
    p, g, m, v = (x[k].to(DEV) for k in ("p", "g", "m", "v"))
    sqnorm = torch.full((case.sqnorm_len,), oo.SENTINEL, device=DEV)
    step = torch.tensor([case.step0], dtype=torch.long, device=DEV)
    hyper = (oo.LR, oo.B1, oo.B2, oo.EPS, x["max_norm"])
    if case.kind == "f32":
        ext.fused_adam(p, g, m, v, sqnorm, step, *hyper)
        p16 = None
    else:
        p16 = torch.zeros(case.n if case.mirror else 0, dtype=torch.bfloat16, device=DEV)
        if not case.do_prologue:  # the caller's part of the contract
            sqnorm[0] = 0.0
            step += 1
        ext.fused_adam_bf16(p, g, m, v, sqnorm, step, p16, *hyper, case.grad_scale,
                            case.do_prologue)
        p16 = p16.cpu()
    torch.cuda.synchronize()
    return {"p": p.cpu(), "m": m.cpu(), "v": v.cpu(), "step": step.cpu(),
            "sqnorm": sqnorm.cpu(), "p16": p16}


@pytest.mark.parametrize("case", oo.CASES, ids=lambda c: c.id)
def test_one_step_against_float64(ext, case):
    x = oo.make_inputs(case)
    oo.check(case, x, run(ext, case, x), "hip")


def test_report_ratios():
    for key in sorted(oo.RATIOS):
        if key.startswith("hip:"):
            print(f"max error/bound {key} = {oo.RATIOS[key]:.4f}")
