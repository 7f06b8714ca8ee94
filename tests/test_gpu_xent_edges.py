"""Linear + label-smoothed CE on MI355X, every kernel family
(csrc/kernels/linear_xent.hip impl 2 / 1 / 0, linear_xent_wide.hip,
linear_xent_mfma.hip), at chosen numbers of valid tokens and at the edges of
V, per row against the float64 oracle of tests/xent_oracle.py:

    row_err(kernel) <= max(8 x row_err(yardstick), 2^-20)

The yardstick is ``ops.reference.linear_xent`` in float32 for the exact-f32
kernels, and the 3-pass bf16 emulation ``xent_oracle.emulate_x3`` for
``linear_xent`` impl 2."""
import contextlib

import pytest
import torch

from tdfo_amd import ops
from tests import xent_oracle as xo

pytestmark = pytest.mark.gpu
DEV = "cuda"
IMPLS = (2, 1, 0)             # 3-pass bf16 MFMA, f32 MFMA, VALU
FILL = 9.0


@pytest.fixture(scope="module", autouse=True)
def _native():
    from tdfo_amd.ops import _ext

    assert _ext.load(), "native library must load on the GPU box"


@contextlib.contextmanager
def _impl(impl):
    before = ops.linear_xent_impl(-1)
    try:
        if impl is not None:
            ops.linear_xent_impl(impl)
            assert ops.linear_xent_impl(-1) == impl
        yield
    finally:
        ops.linear_xent_impl(before)
    assert ops.linear_xent_impl(-1) == before


def _run(case, with_loss=True):
    """ops.linear_xent on device copies of the case -> [dH, lossv, dW, db, mean
    loss]; every output pre-filled with FILL."""
    H, W, b, y = case.inputs
    N, E = H.shape
    V = W.shape[0]
    out = [torch.full((N, E), FILL, device=DEV), torch.full((N,), FILL, device=DEV),
           torch.full((V, E), FILL, device=DEV), torch.full((V,), FILL, device=DEV)]
    loss = torch.full((1,), FILL, device=DEV) if with_loss else None
    ops.linear_xent(H.to(DEV), W.to(DEV), b.to(DEV), y.to(DEV), case.eps, case.ignore, *out,
                    loss=loss)
    torch.cuda.synchronize()
    return out + ([loss[0]] if with_loss else [])


def _check(case, E, impl, tag):
    with _impl(impl):
        out = _run(case)
    xo.assert_within(out, case, xo.yardstick(E, impl), tag)
    ign = case.inputs[3] == case.ignore
    assert float(out[0].cpu()[ign].abs().sum()) == 0 and float(out[1].cpu()[ign].abs().sum()) == 0
    return out


@pytest.mark.parametrize("impl", IMPLS)
@pytest.mark.parametrize("nv,N,layout", xo.NV16_CASES)
def test_e16_chosen_nv(nv, N, layout, impl):
    """E = 16: ng = 1 .. 8 groups in the first block, a last block of 1 and of
    8 groups, nv % 16 in {0, 1, 15}, the 96 / 97 and 128 / 129 thresholds, the
    second pass of the compaction loop (N = 1030, "back")."""
    case = xo.nv_case(xo.NV16_V, N, nv, 16, layout)
    _check(case, 16, impl, f"E=16 impl={impl} V={xo.NV16_V} N={N} nv={nv} {layout}")


@pytest.mark.parametrize("impl", IMPLS)
@pytest.mark.parametrize("nv", xo.V_EDGE_NV)
@pytest.mark.parametrize("V", xo.V_EDGES)
def test_e16_vocab_edges(V, nv, impl):
    """E = 16: no ragged tile, only the ragged tile, odd and even counts of
    full tiles, two tiles per wgrad wave (V = 70001); labels on row V - 1 and
    on the first row of the last full tile."""
    _check(xo.edge_case(V, nv, 16), 16, impl, f"E=16 impl={impl} V={V} nv={nv}")


@pytest.mark.parametrize("E", (32, 64))
@pytest.mark.parametrize("nv", xo.WIDE_NV)
@pytest.mark.parametrize("V", xo.WIDE_V)
def test_wide_edges(V, nv, E):
    _check(xo.edge_case(V, nv, E), E, None, f"E={E} V={V} nv={nv}")


@pytest.mark.parametrize("E", xo.WIDTHS)
@pytest.mark.parametrize("nv", xo.MFMA_NV)
@pytest.mark.parametrize("V", xo.MFMA_V)
def test_mfma_edges(V, nv, E):
    _check(xo.edge_case(V, nv, E), E, None, f"E={E} V={V} nv={nv}")


@pytest.mark.parametrize("E,impl", [(16, 2), (16, 1), (16, 0), (32, None), (64, None),
                                    (128, None), (256, None)])
@pytest.mark.parametrize("family", xo.FAMILIES)
def test_input_families(family, E, impl):
    """randn, H x 12, one hot label, a fitted output layer (p_y > 0.999),
    eps = 0, and ignore = -100 with labels equal to 0."""
    _check(xo.family_case(family, E), E, impl, f"{family} E={E} impl={impl}")


@pytest.mark.parametrize("E,impl", [(16, 2), (16, 1), (16, 0), (32, None), (64, None),
                                    (128, None), (256, None)])
@pytest.mark.parametrize("nv", (97, 257))
def test_two_calls_bit_identical(nv, E, impl):
    case = xo.nv_case(1000, nv + 7, nv, E)
    with _impl(impl):
        a, b = _run(case), _run(case)
    for k, x, z in zip(xo.NAMES5, a, b):
        assert torch.equal(x, z), k


@pytest.mark.parametrize("impl", (2, 1))
@pytest.mark.parametrize("nv", (129, 257))
def test_loss_path_equals_no_loss_path(nv, impl):
    """With ``loss=`` the slab sum runs in xent_tail_kernel, without it in
    xent_slab_reduce_kernel: the same dW / db bits (and dH, lossv)."""
    case = xo.nv_case(xo.NV16_V, nv + 7, nv, 16)
    with _impl(impl):
        a, b = _run(case, True), _run(case, False)
    for k, x, z in zip(xo.NAMES, a, b):
        assert torch.equal(x, z), k
    xo.assert_within(b + [a[4]], case, xo.yardstick(16, impl), f"no loss= impl={impl} nv={nv}")


@pytest.mark.parametrize("impl", IMPLS)
@pytest.mark.parametrize("opt", [ops.OPT_ADAM, ops.OPT_ADAMW])
@pytest.mark.parametrize("nv", (96, 97, 128, 129))
def test_fused_step_at_chosen_nv(nv, opt, impl):
    """The fused output-layer step on both sides of NG <= 6 (the Adam-moment
    prefetch) and of nv <= 128 (wgrad epilogue / slab sum): equal to
    linear_xent + the flat dense optimizer, bit for bit."""
    V, E = xo.NV16_V, 16
    H, W, b, y = (t.to(DEV) for t in xo.make_nv_case(V, nv + 7, nv, E, "spread"))
    N = H.shape[0]
    g = torch.Generator().manual_seed(nv)
    pad = -(-V // 64) * 64                    # flat-buffer padding (optim/flat.py ALIGN)
    mom = [torch.rand(V * E, generator=g).to(DEV), torch.rand(V * E, generator=g).to(DEV),
           torch.rand(pad, generator=g).to(DEV), torch.rand(pad, generator=g).to(DEV)]
    hyper = torch.tensor([1e-3, 7.0, 1.0], device=DEV)
    prm = (0.9, 0.999, 1e-8, 1e-2)
    with _impl(impl):
        Wa, ba = W.clone(), torch.zeros(pad, device=DEV)
        ba[:V] = b
        ma = [m.clone() for m in mom]
        dH, lv, dW, db = (torch.zeros(N, E, device=DEV), torch.zeros(N, device=DEV),
                          torch.zeros(V, E, device=DEV), torch.zeros(pad, device=DEV))
        ops.linear_xent(H, Wa, ba[:V], y, xo.EPS, xo.IGNORE, dH, lv, dW, db[:V])
        ops.dense_optimizer(Wa.view(-1), dW.view(-1), ma[0], ma[1], None, opt, hyper, *prm)
        ops.dense_optimizer(ba, db, ma[2], ma[3], None, opt, hyper, *prm)
        Wb, bb = W.clone(), torch.zeros(pad, device=DEV)
        bb[:V] = b
        mb = [m.clone() for m in mom]
        dH2, lv2 = torch.zeros(N, E, device=DEV), torch.zeros(N, device=DEV)
        ops.linear_xent(H, Wb, bb[:V], y, xo.EPS, xo.IGNORE, dH2, lv2,
                        torch.zeros(V, E, device=DEV), torch.zeros(V, device=DEV),
                        step=(opt, [mb[0], mb[1], mb[2][:V], mb[3][:V]], hyper, *prm))
        torch.cuda.synchronize()
    assert torch.equal(dH, dH2) and torch.equal(lv, lv2)
    assert torch.equal(Wa, Wb) and not torch.equal(Wa, W)
    assert torch.equal(ba[:V], bb[:V])
    for x, z in zip(ma, mb):
        k = V * E if x.numel() == V * E else V
        assert torch.equal(x[:k], z[:k])
