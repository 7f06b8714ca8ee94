"""Linear + label-smoothed CE at hidden 128 / 256 (csrc/kernels/linear_xent_mfma.hip)
on MI355X against the float64 oracle of tests/xent_oracle.py."""
import pytest
import torch

from tdfo_amd import ops
from tests import xent_oracle as xo

pytestmark = pytest.mark.gpu
DEV = "cuda"


@pytest.fixture(scope="module", autouse=True)
def _native():
    from tdfo_amd.ops import _ext

    assert _ext.load(), "native library must load on the GPU box"


def _run(H, W, b, y, with_loss=False):
    """ops.linear_xent on device copies -> [dH, lossv, dW, db] (+ loss)"""
    N, E = H.shape
    V = W.shape[0]
    out = [torch.zeros(N, E, device=DEV), torch.zeros(N, device=DEV),
           torch.zeros(V, E, device=DEV), torch.zeros(V, device=DEV)]
    loss = torch.zeros(1, device=DEV) if with_loss else None
    ops.linear_xent(H.to(DEV), W.to(DEV), b.to(DEV), y.to(DEV), xo.EPS, xo.IGNORE, *out, loss=loss)
    torch.cuda.synchronize()
    return out + ([loss] if with_loss else [])


def _check(out, want, tag):
    errs = {k: xo.rel_err(a, r) for k, a, r in zip(xo.NAMES + ("mean",), out, want)}
    print(f"kernel vs fp64 {tag}: " + " ".join(f"{k}={v:.2e}" for k, v in errs.items()))
    for k, v in errs.items():
        assert v < xo.BOUND, (tag, k, v)


@pytest.mark.parametrize("E", xo.WIDTHS)
@pytest.mark.parametrize("V,N,hs", xo.CASES)
def test_kernel_matches_fp64_oracle(V, N, hs, E):
    """dH, per-token loss, dW, db and the mean loss within 2e-4 of fp64."""
    out = _run(*xo.make_case(V, N, hs, E), with_loss=True)
    out[4] = out[4][0]
    _check(out, xo.oracle_case(V, N, hs, E), f"V={V} N={N} hs={hs} E={E}")


@pytest.mark.parametrize("E", xo.WIDTHS)
@pytest.mark.parametrize("V,N", xo.SPLIT_CASES)
def test_forced_splits(V, N, E):
    """Every split count (some leave a split with less than one W tile) is
    within the bound, two runs at one count are bit-identical, and the hook
    restores."""
    case = xo.make_case(V, N, 1.0, E)
    want = xo.oracle_case(V, N, 1.0, E)
    before = ops.linear_xent_splits(-1)
    try:
        for n in (1, 2, 3, 7):
            prev = ops.linear_xent_splits(n)
            assert ops.linear_xent_splits(-1) == n
            a = _run(*case)
            b = _run(*case)
            for x, z in zip(a, b):
                assert torch.equal(x, z), n
            _check(a, want[:4], f"V={V} N={N} E={E} splits={n}")
            assert ops.linear_xent_splits(prev) == n
    finally:
        ops.linear_xent_splits(before)
    assert ops.linear_xent_splits(-1) == before


@pytest.mark.parametrize("E", xo.WIDTHS)
@pytest.mark.parametrize("opt", [ops.OPT_ADAM, ops.OPT_ADAMW])
@pytest.mark.parametrize("V,N", [(4099, 320), (5003, 1030), (100, 64)])
def test_fused_step_matches_separate_optimizer(V, N, opt, E):
    """The output layer's Adam / AdamW step after wgrad equals linear_xent +
    the flat dense optimizer, bit for bit; (100, 64) has every label ignored:
    the zero-gradient step."""
    torch.manual_seed(V + N + E)
    H = torch.randn(N, E, device=DEV)
    W = torch.randn(V, E, device=DEV) * 0.2
    b = torch.randn(V, device=DEV) * 0.1
    y = torch.randint(1, V, (N,), device=DEV)
    y[torch.rand(N, device=DEV) < 0.6] = 0
    if V == 100:
        y.zero_()
    pad = -(-V // 64) * 64                    # flat-buffer padding (optim/flat.py ALIGN)
    mom = [torch.rand(V * E, device=DEV), torch.rand(V * E, device=DEV),
           torch.rand(pad, device=DEV), torch.rand(pad, device=DEV)]
    hyper = torch.tensor([1e-3, 7.0, 1.0], device=DEV)
    prm = (0.9, 0.999, 1e-8, 1e-2)
    # separate: gradient, then the flat optimizer on W and bias
    Wa, ba = W.clone(), torch.zeros(pad, device=DEV)
    ba[:V] = b
    ma = [m.clone() for m in mom]
    dH, lv, dW, db = (torch.zeros(N, E, device=DEV), torch.zeros(N, device=DEV),
                      torch.zeros(V, E, device=DEV), torch.zeros(pad, device=DEV))
    ops.linear_xent(H, Wa, ba[:V], y, 0.1, 0, dH, lv, dW, db[:V])
    ops.dense_optimizer(Wa.view(-1), dW.view(-1), ma[0], ma[1], None, opt, hyper, *prm)
    ops.dense_optimizer(ba, db, ma[2], ma[3], None, opt, hyper, *prm)
    # fused
    Wb, bb = W.clone(), torch.zeros(pad, device=DEV)
    bb[:V] = b
    mb = [m.clone() for m in mom]
    dH2, lv2 = torch.zeros(N, E, device=DEV), torch.zeros(N, device=DEV)
    db2 = torch.zeros(pad, device=DEV)
    ops.linear_xent(H, Wb, bb[:V], y, 0.1, 0, dH2, lv2, torch.zeros(V, E, device=DEV), db2[:V],
                    step=(opt, [mb[0], mb[1], mb[2][:V], mb[3][:V]], hyper, *prm))
    torch.cuda.synchronize()
    assert torch.equal(dH, dH2) and torch.equal(lv, lv2)
    assert torch.equal(Wa, Wb)
    assert not torch.equal(Wa, W)             # (a step was taken: AdamW decay, Adam's L2 term)
    assert torch.equal(ba[:V], bb[:V])
    for x, z in zip(ma, mb):
        k = V * E if x.numel() == V * E else V
        assert torch.equal(x[:k], z[:k])


@pytest.mark.parametrize("E", xo.WIDTHS)
def test_all_ignored(E):
    N, V = 64, 100
    H = torch.randn(N, E, device=DEV)
    W = torch.randn(V, E, device=DEV)
    b = torch.zeros(V, device=DEV)
    y = torch.zeros(N, dtype=torch.int64, device=DEV)
    dH, lv = torch.ones(N, E, device=DEV), torch.ones(N, device=DEV)
    dW, db = torch.ones(V, E, device=DEV), torch.ones(V, device=DEV)
    loss = torch.ones(1, device=DEV)
    ops.linear_xent(H, W, b, y, 0.1, 0, dH, lv, dW, db, loss=loss)
    torch.cuda.synchronize()
    assert float(dH.abs().sum()) == 0 and float(lv.abs().sum()) == 0
    assert float(dW.abs().sum()) == 0 and float(db.abs().sum()) == 0
    assert float(loss) == 0


@pytest.mark.parametrize("E", xo.WIDTHS)
def test_no_tokens(E):
    """N = 0: nothing is launched, so nothing is written (dW / db keep their
    fill) and nothing faults."""
    V = 100
    W = torch.randn(V, E, device=DEV)
    dW, db = torch.ones(V, E, device=DEV), torch.ones(V, device=DEV)
    loss = torch.full((1,), 5.0, device=DEV)
    ops.linear_xent(torch.zeros(0, E, device=DEV), W, torch.zeros(V, device=DEV),
                    torch.zeros(0, dtype=torch.int64, device=DEV), 0.1, 0,
                    torch.zeros(0, E, device=DEV), torch.zeros(0, device=DEV), dW, db, loss=loss)
    torch.cuda.synchronize()
    assert bool((dW == 1).all()) and bool((db == 1).all()) and float(loss) == 5.0


def test_no_logits_in_hbm():
    """The call's peak allocation stays under a quarter of an [N, V] fp32
    logits tensor (dW / db are the caller's)."""
    V, N, E = 200_000, 512, 128
    g = torch.Generator().manual_seed(5)
    H = torch.randn(N, E, generator=g).to(DEV)
    W = (torch.randn(V, E, generator=g) * 0.2).to(DEV)
    b = torch.zeros(V, device=DEV)
    y = torch.randint(1, V, (N,), generator=g).to(DEV)
    out = [torch.zeros(N, E, device=DEV), torch.zeros(N, device=DEV),
           torch.zeros(V, E, device=DEV), torch.zeros(V, device=DEV)]
    ops.linear_xent(H, W, b, y, 0.1, 0, *out)              # warm-up
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.max_memory_allocated()
    ops.linear_xent(H, W, b, y, 0.1, 0, *out)
    torch.cuda.synchronize()
    grew = torch.cuda.max_memory_allocated() - base
    print(f"peak allocation across the call: {grew} bytes; logits would be {N * V * 4}")
    assert grew < N * V * 4 // 4
    assert bool(torch.isfinite(out[1]).all()) and float(out[1].min()) > 0


@pytest.mark.parametrize("E", [16, 32, 64])
def test_existing_widths_untouched(E):
    """The split hook and the new dispatch do not reach E = 16 / 32 / 64: the
    same bits with the hook forced to 1 and to 3."""
    V, N = 4099, 320
    g = torch.Generator().manual_seed(E)
    case = (torch.randn(N, E, generator=g), torch.randn(V, E, generator=g) * 0.2,
            torch.randn(V, generator=g) * 0.1, torch.randint(0, V, (N,), generator=g))
    force = getattr(ops, "linear_xent_splits", lambda n=-1: 0)    # (absent: nothing to reach)
    before = force(-1)
    try:
        force(1)
        a = _run(*case, with_loss=True)
        force(3)
        b = _run(*case, with_loss=True)
    finally:
        force(before)
    for x, z in zip(a, b):
        assert torch.equal(x, z)
    ref = [torch.zeros(N, E), torch.zeros(N), torch.zeros(V, E), torch.zeros(V)]
    ops.reference.linear_xent(*case, xo.EPS, xo.IGNORE, *ref)
    for k, x, r in zip(xo.NAMES, a, ref):
        assert xo.rel_err(x, r) < xo.BOUND, k


@pytest.mark.parametrize("E", [96, 512])
def test_host_side_width_check(E):
    """An unsupported width raises on the host, nothing is launched (the
    outputs keep their fill), and a valid call afterwards passes."""
    V, N = 50, 7
    dH, lv = torch.ones(N, E, device=DEV), torch.ones(N, device=DEV)
    dW, db = torch.ones(V, E, device=DEV), torch.ones(V, device=DEV)
    with pytest.raises(RuntimeError, match="128"):
        ops.linear_xent(torch.randn(N, E, device=DEV), torch.randn(V, E, device=DEV),
                        torch.zeros(V, device=DEV), torch.ones(N, dtype=torch.int64, device=DEV),
                        0.1, 0, dH, lv, dW, db)
    torch.cuda.synchronize()
    for t in (dH, lv, dW, db):
        assert bool((t == 1).all())
    out = _run(*xo.make_case(V, N, 1.0, 128))
    _check(out, xo.oracle_case(V, N, 1.0, 128)[:4], "after a refused call")
