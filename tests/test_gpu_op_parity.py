"""GPU (-m gpu): every pointwise / gather / reduction kernel of the GMFlow and GMFSS glue on its own against a float64
reference (tests/op_checks.py), at the sizes where kernels go wrong: image borders, partial tiles and blocks, every dispatch
branch, batch > 1, grid-stride loops that go round twice.  One operator family per test, so that a failure names it.

Value rows: tol = max(2e-5 max(1, |ref|max), 3 x the fp32 oracle's own error on that input); decisions and data movement:
bit-exact.  tests/test_op_checks_cpu.py shows on the CPU that these rows fail for a wrong operator."""
import pytest
import torch

from tests import op_checks, report

pytestmark = pytest.mark.gpu


def _assert_rows(rows):
    import inspect
    report.record(inspect.stack()[1].function, rows)
    for n, e, t, x in rows:
        print(f"  {n:58s} err={e:.3e} tol={t:.1e} {x}")
    bad = [(n, e, t, x) for n, e, t, x in rows if not e <= t]
    assert not bad, "\n".join(f"{n}: err={e:.3e} tol={t:.1e} {x}" for n, e, t, x in bad)


def test_softmax_rows(hip_backend):
    _assert_rows(op_checks.check_softmax_rows(hip_backend.dev))


def test_instance_norm(hip_backend):
    _assert_rows(op_checks.check_instance_norm(hip_backend.dev))


def test_conv_direct(hip_backend):
    _assert_rows(op_checks.check_conv_direct(hip_backend.dev))


def test_local_corr_flow(hip_backend):
    _assert_rows(op_checks.check_local_corr_flow(hip_backend.dev))


def test_local_attn_flow(hip_backend):
    _assert_rows(op_checks.check_local_attn_flow(hip_backend.dev))


def test_convex_upsample(hip_backend):
    _assert_rows(op_checks.check_convex_upsample(hip_backend.dev))


def test_flow_warp(hip_backend):
    _assert_rows(op_checks.check_flow_warp(hip_backend.dev))


def test_backwarp(hip_backend):
    _assert_rows(op_checks.check_backwarp(hip_backend.dev))


def test_resize_bilinear_ac(hip_backend):
    _assert_rows(op_checks.check_resize_bilinear_ac(hip_backend.dev))


def test_layernorm(hip_backend):
    _assert_rows(op_checks.check_layernorm(hip_backend.dev))


def test_gelu(hip_backend):
    _assert_rows(op_checks.check_gelu(hip_backend.dev))


def test_bmm(hip_backend):
    _assert_rows(op_checks.check_bmm(hip_backend.dev))


def test_pointwise(hip_backend):
    _assert_rows(op_checks.check_pointwise(hip_backend.dev))


def test_layouts(hip_backend):
    _assert_rows(op_checks.check_layouts(hip_backend.dev))


def test_hole_tests(hip_backend):
    _assert_rows(op_checks.check_hole_tests(hip_backend.dev))


def test_drm_ratio_and_retime(hip_backend):
    _assert_rows(op_checks.check_drm(hip_backend.dev))


def test_metric_input(hip_backend):
    _assert_rows(op_checks.check_metric_input(hip_backend.dev))


def test_documented_refusals(hip_backend):
    """Shapes a launcher documents as refused raise DrbaHipError; nothing is launched for them."""
    from drba_amd import _lib, ops
    dev = hip_backend.dev
    z = lambda *s: torch.zeros(*s, device=dev)  # noqa: E731
    for radius in (1, 3, 5):  # only the radius GMFlow's refinement stage uses
        with pytest.raises(_lib.DrbaHipError):
            ops.local_corr_flow(z(1, 128, 8, 8), z(1, 128, 8, 8), radius)
    for h, w in ((1, 8), (8, 1), (1, 1)):  # 2c / (n - 1) - 1 has no meaning for n = 1
        with pytest.raises(_lib.DrbaHipError):
            ops.flow_warp(z(1, 4, h, w), z(1, 2, h, w))
        with pytest.raises(_lib.DrbaHipError):
            ops.backwarp(z(1, 4, h, w), z(1, 2, h, w), "zeros")
        with pytest.raises(_lib.DrbaHipError):
            ops.metric_input(z(1, 3, h, w), z(1, 3, h, w), z(1, 2, h, w), z(1, 2, h, w))
    with pytest.raises(_lib.DrbaHipError):
        ops.softmax_rows_(z(2, 3, 5), 0.0)  # scale must be positive
    torch.cuda.synchronize()
