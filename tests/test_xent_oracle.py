"""The fp32 reference of Linear + label-smoothed CE against the float64 oracle
(tests/xent_oracle.py), at every shape the GPU test of the hidden 128 / 256
kernels uses: the 2e-4 bound asked of those kernels leaves the fp32 reference
itself a wide margin."""
import pytest
import torch

from tdfo_amd import ops
from tests import xent_oracle as xo


def test_oracle_matches_autograd_fp64():
    """The hand-written oracle against torch autograd in fp64 on a tiny case."""
    H, W, b, y = xo.make_case(50, 7, 1.0, 128)
    dH, lv, dW, db, mean = xo.oracle(H, W, b, y)
    Hd, Wd, bd = (t.double().requires_grad_(True) for t in (H, W, b))
    per = torch.nn.functional.cross_entropy(Hd @ Wd.t() + bd, y, ignore_index=xo.IGNORE,
                                            label_smoothing=xo.EPS, reduction="none")
    m = per.sum() / max(1, int((y != xo.IGNORE).sum()))
    m.backward()
    for a, r in ((dH, Hd.grad), (lv, per.detach()), (dW, Wd.grad), (db, bd.grad), (mean, m.detach())):
        assert xo.rel_err(a, r) < 1e-12


@pytest.mark.parametrize("E", xo.WIDTHS)
@pytest.mark.parametrize("V,N,hs", xo.CASES)
def test_fp32_reference_within_bound(V, N, hs, E):
    H, W, b, y = xo.make_case(V, N, hs, E)
    out = [torch.zeros(N, E), torch.zeros(N), torch.zeros(V, E), torch.zeros(V)]
    ops.reference.linear_xent(H, W, b, y, xo.EPS, xo.IGNORE, *out)
    want = xo.oracle_case(V, N, hs, E)
    nv = max(1, int((y != xo.IGNORE).sum()))
    errs = {k: xo.rel_err(a, r) for k, a, r in zip(xo.NAMES, out, want)}
    errs["mean"] = xo.rel_err(out[1].sum() / nv, want[4])
    print(f"fp32 reference vs fp64 V={V} N={N} hs={hs} E={E}: "
          + " ".join(f"{k}={v:.2e}" for k, v in errs.items()))
    for k, v in errs.items():
        assert v < xo.BOUND, (k, v)
