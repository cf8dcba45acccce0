"""The fused clip + Adam formula evaluated in float32 torch on the CPU,
against the float64 reference and the derived bounds of
tests/optim_oracle.py, for every case tests/test_optim_gpu.py runs on the
kernels. A bound that the plain float32 evaluation cannot meet is wrong."""
import pytest

import optim_oracle as oo


@pytest.mark.parametrize("case", oo.CASES, ids=lambda c: c.id)
def test_float32_formula_within_bounds(case):
    x = oo.make_inputs(case)
    oo.check(case, x, oo.torch32_step(case, x), "torch32")


def test_report_ratios():
    for key in sorted(oo.RATIOS):
        if key.startswith("torch32:"):
            print(f"max error/bound {key} = {oo.RATIOS[key]:.4f}")
