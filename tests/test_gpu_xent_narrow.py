"""Linear + label-smoothed CE at hidden 16 / 32 / 64 (csrc/kernels/linear_xent.hip
and linear_xent_wide.hip) on MI355X against the float64 oracle of
tests/xent_oracle.py: the cases and the 2e-4 bound of the hidden 128 / 256
test, E = 16 under each kernel family (ops.linear_xent_impl 2, 1, 0), and per
row under max(8 x row_err(yardstick), 2^-20) (xent_oracle.assert_within)."""
import pytest
import torch

from tdfo_amd import ops
from tests import xent_oracle as xo

pytestmark = pytest.mark.gpu
DEV = "cuda"
IMPLS = {16: (2, 1, 0), 32: (None,), 64: (None,)}      # 3-pass bf16 MFMA, f32 MFMA, VALU


@pytest.fixture(scope="module", autouse=True)
def _native():
    from tdfo_amd.ops import _ext

    assert _ext.load(), "native library must load on the GPU box"


def _run(H, W, b, y):
    """ops.linear_xent on device copies -> [dH, lossv, dW, db, mean loss]"""
    N, E = H.shape
    V = W.shape[0]
    out = [torch.full((N, E), 9.0, device=DEV), torch.full((N,), 9.0, device=DEV),
           torch.full((V, E), 9.0, device=DEV), torch.full((V,), 9.0, device=DEV)]
    loss = torch.full((1,), 9.0, device=DEV)
    ops.linear_xent(H.to(DEV), W.to(DEV), b.to(DEV), y.to(DEV), xo.EPS, xo.IGNORE, *out, loss=loss)
    torch.cuda.synchronize()
    return out + [loss[0]]


@pytest.mark.parametrize("E,impl", [(E, i) for E in xo.NARROW_WIDTHS for i in IMPLS[E]])
@pytest.mark.parametrize("V,N,hs", xo.CASES)
def test_narrow_kernel_matches_fp64_oracle(V, N, hs, E, impl):
    """dH, per-token loss, dW, db and the mean loss (through ``loss=``) within
    2e-4 of fp64, and dH / dW per row, lossv / db per element and the mean
    within 8 x the error of the family's yardstick: the fp32 reference, or
    the 3-pass emulation for impl 2."""
    case, want = xo.make_case(V, N, hs, E), xo.oracle_case(V, N, hs, E)
    before = ops.linear_xent_impl(-1)
    try:
        if impl is not None:
            ops.linear_xent_impl(impl)
            assert ops.linear_xent_impl(-1) == impl
        out = _run(*case)
    finally:
        ops.linear_xent_impl(before)
    assert ops.linear_xent_impl(-1) == before
    tag = f"V={V} N={N} hs={hs} E={E} impl={impl}"
    errs = {k: xo.rel_err(a, r) for k, a, r in zip(xo.NAMES + ("mean",), out, want)}
    print(f"kernel vs fp64 {tag}: " + " ".join(f"{k}={v:.2e}" for k, v in errs.items()))
    for k, v in errs.items():
        assert v < xo.BOUND, (tag, k, v)
    xo.assert_within(out, xo.random_case(V, N, hs, E), xo.yardstick(E, impl), tag)
    ign = case[3] == xo.IGNORE
    assert float(out[0].cpu()[ign].abs().sum()) == 0 and float(out[1].cpu()[ign].abs().sum()) == 0
