"""The float32 torch branch of ops/multistep.py, on the CPU, against the
float64 references and rounding bounds of tests/scan_oracle.py: the same
inputs, shapes and bounds that tests/test_scan_gpu.py holds the HIP kernels
to. A bound the plain float32 evaluation cannot meet would be a wrong bound."""
import pytest

import scan_oracle as so


@pytest.mark.parametrize("T,B", so.SHAPES, ids=lambda v: str(v))
def test_cpu_branch_within_rounding_bound(T, B):
    so.run_all(T, B, "cpu", seed=1000 * T + B)


def test_cpu_branch_undamped_transposed_trailing_and_broadcast():
    x = so.make_inputs(37, 65, seed=7, undamped=True)
    so.check_gae(x, 1.0, "cpu")
    so.check_lambda_returns(x, 1.0, "cpu")
    so.check_vtrace(x, 1.0, 1.0, 1.0, "cpu")
    so.check_retrace(x, 1.0, "cpu")

    x = so.make_inputs(37, 65, seed=11)
    so.check_gae(x, 0.95, "cpu", view=so.transposed)
    so.check_lambda_returns(x, 0.95, "cpu", view=so.transposed)
    so.check_vtrace(x, 0.9, 0.8, 1.5, "cpu", view=so.transposed)
    so.check_offpolicy(x, "cpu", view=so.transposed)
    so.check_retrace(x, 0.95, "cpu", view=so.transposed)

    T, B = 7, 43
    x = so.make_inputs(T, B * 3, seed=13)
    view = lambda key, t: t.reshape(T, B, 3)
    flat = (T, B * 3)
    so.check_gae(x, 0.95, "cpu", view=view, shape=flat)
    so.check_lambda_returns(x, 0.95, "cpu", view=view, shape=flat)
    so.check_vtrace(x, 0.9, 0.8, 1.5, "cpu", view=view, shape=flat)
    so.check_offpolicy(x, "cpu", view=view, shape=flat)

    T, B = 9, 130
    x = so.make_inputs(T, B, seed=17)
    x["d"] = x["d"][:, :1].expand(T, B).contiguous()
    view = lambda key, t: t[:, :1].contiguous() if key == "d" else t
    so.check_gae(x, 0.95, "cpu", view=view)
    so.check_lambda_returns(x, 0.95, "cpu", view=view)
    so.check_vtrace(x, 0.9, 0.8, 1.5, "cpu", view=view)
    so.check_offpolicy(x, "cpu", view=view)
    for key in sorted(so.RATIOS):
        if key.startswith("cpu:"):
            print(f"max error/bound {key} = {so.RATIOS[key]:.4f}")
