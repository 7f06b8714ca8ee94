"""Shared-negative Linear + BCE / gBCE (csrc/kernels/linear_bce_rows.hip) and
its candidate builder on MI355X, against the float64 oracle of
tests/bce_rows_oracle.py."""
import pytest
import torch

from tdfo_amd import ops
from tests import bce_rows_oracle as bo

pytestmark = pytest.mark.gpu
DEV = "cuda"
FILL = 1.0


@pytest.fixture(scope="module", autouse=True)
def _native():
    from tdfo_amd.ops import _ext

    assert _ext.load(), "native library must load on the GPU box"


def _run(H, W, b, labels, order, negs, beta=1.0, ignore=bo.IGNORE):
    """ops.linear_bce_rows on device copies -> [dH, lossv, dW, db, loss];
    dW / db are pre-filled with FILL."""
    N, E = H.shape
    V = W.shape[0]
    out = [torch.zeros(N, E, device=DEV), torch.zeros(N, device=DEV),
           torch.full((V, E), FILL, device=DEV), torch.full((V,), FILL, device=DEV)]
    loss = torch.zeros(1, device=DEV)
    ops.linear_bce_rows(H.to(DEV), W.to(DEV), b.to(DEV), labels.to(DEV), order.to(DEV),
                        negs.to(DEV), beta, ignore, *out, loss=loss)
    torch.cuda.synchronize()
    return out + [loss]


def _check(out, want, labels, negs, V, tag):
    """Every output within BOUND of fp64 on the rows the call owns; every
    other row of dW / db still holds its fill, exactly."""
    named = bo.named_rows(labels, negs, V)
    dW, db = out[2].cpu(), out[3].cpu()
    assert bool((dW[~named] == FILL).all()) and bool((db[~named] == FILL).all()), tag
    got = [out[0], out[1], dW[named], db[named], out[4][0]]
    ref = [want[0], want[1], want[2][named], want[3][named], want[4]]
    errs = {k: bo.rel_err(a, r) for k, a, r in zip(bo.NAMES, got, ref)}
    print(f"kernel vs fp64 {tag}: " + " ".join(f"{k}={v:.2e}" for k, v in errs.items()))
    for k, v in errs.items():
        assert v < bo.BOUND, (tag, k, v)


@pytest.mark.parametrize("E", bo.WIDTHS)
def test_kernel_matches_fp64_oracle(E):
    """dH, per-token loss, dW, db and the mean loss within 2e-4 of fp64 at
    every case, for beta 1.0 and 0.3."""
    for N, S, V, hs in bo.CASES:
        case = bo.make_case(N, S, E, V, hs)
        for beta in bo.BETAS:
            out = _run(*case, beta=beta)
            _check(out, bo.oracle_case(N, S, E, V, hs, beta), case[3], case[5], V,
                   f"N={N} S={S} V={V} hs={hs} beta={beta} E={E}")


@pytest.mark.parametrize("E", bo.WIDTHS)
def test_holes_are_free(E):
    """A call with holes equals, bit for bit, the call with the holes removed;
    two identical calls are bit-identical."""
    for N, S in [(320, 513), (65, 64)]:
        H, W, b, labels, order, negs = bo.make_case(N, S, E)
        a = _run(H, W, b, labels, order, negs, 0.3)
        a2 = _run(H, W, b, labels, order, negs, 0.3)
        dense = bo.valid_negs(negs, bo.V).contiguous()
        assert dense.numel() < S
        c = _run(H, W, b, labels, order, dense, 0.3)
        for x, y, z in zip(a, a2, c):
            assert torch.equal(x, y), (N, S)
            assert torch.equal(x, z), (N, S)


@pytest.mark.parametrize("E", bo.WIDTHS)
def test_token_splits(E):
    """More valid tokens than two splits of the negatives' wgrad (1024 tokens a
    split at E <= 64, 2048 above; the shapes of bce_rows_oracle.CASES all fit
    one): within the bound, and holes stay free, bit for bit. The one hot label
    is a run of about 2700 tokens for the positives' stage."""
    N, S = 11000, 70
    H, W, b, labels, order, negs = bo.make_case(N, S, E)
    nv = int(bo.valid_tokens(labels, bo.V).sum())
    assert nv > 2 * (1024 if E <= 64 else 2048) and N > nv
    a = _run(H, W, b, labels, order, negs, 0.3)
    _check(a, bo.oracle_case(N, S, E, bo.V, 1.0, 0.3), labels, negs, bo.V, f"N={N} S={S} E={E}")
    c = _run(H, W, b, labels, order, bo.valid_negs(negs, bo.V).contiguous(), 0.3)
    for x, z in zip(a, c):
        assert torch.equal(x, z)


@pytest.mark.parametrize("E", bo.WIDTHS)
def test_forced_splits(E):
    """Forced negative splits 1, 2, 3, 7 are each within the bound, and the
    hook restores."""
    N, S = 320, 513
    case = bo.make_case(N, S, E)
    want = bo.oracle_case(N, S, E)
    before = ops.linear_xent_splits(-1)
    try:
        for n in (1, 2, 3, 7):
            prev = ops.linear_xent_splits(n)
            assert ops.linear_xent_splits(-1) == n
            _check(_run(*case), want, case[3], case[5], bo.V, f"N={N} S={S} E={E} splits={n}")
            assert ops.linear_xent_splits(prev) == n
    finally:
        ops.linear_xent_splits(before)
    assert ops.linear_xent_splits(-1) == before


@pytest.mark.parametrize("E", bo.WIDTHS)
def test_hit_equals_negative_removed(E):
    """One token whose label is among the negatives, against the call with
    that negative removed: the same problem."""
    S, V = 130, 400
    g = torch.Generator().manual_seed(E + 1)
    H, W = torch.randn(1, E, generator=g), torch.randn(V, E, generator=g) * 0.2
    b = torch.randn(V, generator=g) * 0.1
    negs = torch.sort(torch.randperm(V - 1, generator=g)[:S] + 1).values
    labels = negs[77:78].clone()
    order = torch.zeros(1, dtype=torch.int32)
    a = _run(H, W, b, labels, order, negs, 0.3)
    c = _run(H, W, b, labels, order, torch.cat([negs[:77], negs[78:]]), 0.3)
    want = bo.oracle(H, W, b, labels, negs, 0.3)
    _check(a, want, labels, negs, V, f"hit E={E}")
    named = bo.named_rows(labels, negs, V).to(DEV)   # (both calls name the same rows)
    for out in (a, c):
        assert bool((out[2][~named] == FILL).all()) and bool((out[3][~named] == FILL).all())
        out[2], out[3] = out[2][named], out[3][named]
    for k, x, z in zip(bo.NAMES, a, c):
        e = bo.rel_err(x, z)
        print(f"hit vs removed E={E} {k}: {e:.2e}")
        assert e < bo.BOUND, k


@pytest.mark.parametrize("E", bo.WIDTHS)
def test_nothing_valid(E):
    """All tokens ignored: zero dH / lossv / loss and nothing written to dW /
    db. All negatives holes with valid tokens: loss_n = beta softplus(-zy),
    only the label rows written, agreement with the oracle."""
    N, S, V, beta = 65, 70, 300, 0.3
    g = torch.Generator().manual_seed(E)
    H, W = torch.randn(N, E, generator=g), torch.randn(V, E, generator=g) * 0.2
    b = torch.randn(V, generator=g) * 0.1
    negs = torch.sort(torch.randperm(V, generator=g)[:S]).values
    ign = torch.tensor([bo.IGNORE, -1, V, V + 3])[torch.arange(N) % 4]
    out = [torch.ones(N, E, device=DEV), torch.ones(N, device=DEV),
           torch.full((V, E), FILL, device=DEV), torch.full((V,), FILL, device=DEV)]
    loss = torch.ones(1, device=DEV)
    ops.linear_bce_rows(H.to(DEV), W.to(DEV), b.to(DEV), ign.to(DEV),
                        bo.label_order(ign, V).to(DEV), negs.to(DEV), beta, bo.IGNORE, *out,
                        loss=loss)
    torch.cuda.synchronize()
    assert float(out[0].abs().sum()) == 0 and float(out[1].abs().sum()) == 0
    assert float(loss) == 0
    assert bool((out[2] == FILL).all()) and bool((out[3] == FILL).all())

    holes = torch.tensor([-1, V, V + 5])[torch.arange(S) % 3]
    labels = torch.randint(1, V, (N,), generator=g)
    labels[:20] = labels[0]
    labels[40:45] = bo.IGNORE
    got = _run(H, W, b, labels, bo.label_order(labels, V), holes, beta)
    want = bo.oracle(H, W, b, labels, holes, beta)
    _check(got, want, labels, holes, V, f"negatives holes E={E}")
    on = bo.valid_tokens(labels, V)
    zy = (H.double() * W.double()[labels]).sum(1) + b.double()[labels]
    sp = beta * ((-zy).clamp_min(0) + torch.log1p(torch.exp(-zy.abs())))
    assert bo.rel_err(got[1].cpu()[on], sp[on]) < bo.BOUND
    named = torch.zeros(V, dtype=torch.bool)
    named[labels[on]] = True
    assert bool((got[2].cpu()[~named] == FILL).all())


@pytest.mark.parametrize("E", bo.WIDTHS)
def test_empty_launches_nothing(E):
    """N = 0 and S = 0: nothing is launched and the outputs keep their fill."""
    V = 100
    W, b = torch.randn(V, E, device=DEV), torch.zeros(V, device=DEV)
    i64 = dict(dtype=torch.int64, device=DEV)
    for N, S in ((0, 5), (7, 0)):
        dH, lv = torch.full((N, E), 3.0, device=DEV), torch.full((N,), 3.0, device=DEV)
        dW, db = torch.full((V, E), FILL, device=DEV), torch.full((V,), FILL, device=DEV)
        loss = torch.full((1,), 5.0, device=DEV)
        ops.linear_bce_rows(torch.randn(N, E, device=DEV), W, b, torch.ones(N, **i64),
                            torch.arange(N, dtype=torch.int32, device=DEV), torch.arange(S, **i64),
                            1.0, 0, dH, lv, dW, db, loss=loss)
        torch.cuda.synchronize()
        assert bool((dH == 3).all()) and bool((lv == 3).all())
        assert bool((dW == FILL).all()) and bool((db == FILL).all()) and float(loss) == 5.0


def test_host_side_width_check():
    """An unsupported width raises on the host naming the supported set,
    nothing is written, and a valid call afterwards passes."""
    V, N, S, E = 50, 7, 9, 96
    dH, lv = torch.ones(N, E, device=DEV), torch.ones(N, device=DEV)
    dW, db = torch.ones(V, E, device=DEV), torch.ones(V, device=DEV)
    i64 = dict(dtype=torch.int64, device=DEV)
    with pytest.raises(RuntimeError, match=r"16\|32\|64\|128\|256"):
        ops.linear_bce_rows(torch.randn(N, E, device=DEV), torch.randn(V, E, device=DEV),
                            torch.zeros(V, device=DEV), torch.ones(N, **i64),
                            torch.arange(N, dtype=torch.int32, device=DEV), torch.arange(S, **i64),
                            1.0, 0, dH, lv, dW, db)
    torch.cuda.synchronize()
    for t in (dH, lv, dW, db):
        assert bool((t == 1).all())
    case = bo.make_case(7, 7, 64)
    _check(_run(*case), bo.oracle_case(7, 7, 64), case[3], case[5], bo.V, "after a refused call")


def test_no_logits_in_hbm():
    """The call's peak allocation stays under a quarter of an [N, S] fp32
    tensor (dW / db are the caller's)."""
    N, S, V, E = 512, 20000, 200_000, 64
    g = torch.Generator().manual_seed(5)
    H = torch.randn(N, E, generator=g).to(DEV)
    W = (torch.randn(V, E, generator=g) * 0.2).to(DEV)
    b = torch.zeros(V, device=DEV)
    negs = torch.sort(torch.randperm(V, generator=g)[:S]).values.to(DEV)
    labels = torch.randint(0, V, (N,), generator=g)
    order = bo.label_order(labels, V, -100).to(DEV)
    labels = labels.to(DEV)
    out = [torch.zeros(N, E, device=DEV), torch.zeros(N, device=DEV),
           torch.zeros(V, E, device=DEV), torch.zeros(V, device=DEV)]
    ops.linear_bce_rows(H, W, b, labels, order, negs, 1.0, -100, *out)  # warm-up
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.max_memory_allocated()
    ops.linear_bce_rows(H, W, b, labels, order, negs, 1.0, -100, *out)
    torch.cuda.synchronize()
    grew = torch.cuda.max_memory_allocated() - base
    print(f"peak allocation across the call: {grew} bytes; logits would be {N * S * 4}")
    assert grew < N * S * 4 // 4
    assert bool(torch.isfinite(out[1]).all()) and float(out[1].min()) > 0


def test_candidate_builder():
    """ops.bce_candidates on the device equals its CPU result exactly."""
    labels, neg = bo.candidate_case()
    neg = neg.clone()
    neg[11], neg[12] = -4, 2 ** 31 + 5
    want = [torch.zeros(neg.numel(), dtype=torch.int64), torch.zeros(labels.numel(),
                                                                    dtype=torch.int32)]
    ops.bce_candidates(labels, neg, 0, *want)
    got = [torch.zeros_like(want[0], device=DEV), torch.zeros_like(want[1], device=DEV)]
    ops.bce_candidates(labels.to(DEV), neg.to(DEV), 0, *got)
    torch.cuda.synchronize()
    assert torch.equal(got[0].cpu(), want[0]) and torch.equal(got[1].cpu(), want[1])
    bo.check_candidates(labels, neg, got[0], got[1], 3002)


# --------------------------------------------- per row, at chosen valid counts
def _per_row(args, tag):
    N, S, E, V, hs, beta, nv, hot = args
    case = bo.make_case(N, S, E, V, hs, nv, hot)
    out = _run(*case, beta=beta)
    named = bo.named_rows(case[3], case[5], V)
    assert bool((out[2].cpu()[~named] == FILL).all()) and bool((out[3].cpu()[~named] == FILL).all())
    bo.assert_within(out[:4] + [out[4][0]], args, tag)
    ign = ~bo.valid_tokens(case[3], V)
    assert int((~ign).sum()) == nv
    assert float(out[0].cpu()[ign].abs().sum()) == 0 and float(out[1].cpu()[ign].abs().sum()) == 0


@pytest.mark.parametrize("E", bo.WIDTHS)
@pytest.mark.parametrize("nv", bo.NV)
def test_chosen_nv_per_row(nv, E):
    """Exactly nv valid tokens: dH and dW per row, lossv and db per element
    and the mean within max(8 x row_err(fp32 reference), 2^-20) of fp64, for
    beta 1.0 and 0.3; unnamed rows keep their fill; ignored tokens get exact
    zeros."""
    N, S = bo.NV_SHAPE
    for beta in bo.BETAS:
        _per_row((N, S, E, bo.V, 1.0, beta, nv, None), f"BCE E={E} N={N} S={S} nv={nv} beta={beta}")


@pytest.mark.parametrize("E", bo.WIDTHS)
@pytest.mark.parametrize("hot", bo.HOT)
def test_hot_run_at_wave_edge(hot, E):
    """The hot label's run is walked by one wave, 64 tokens at a time: runs of
    63, 64 and 65 tokens."""
    N, S = bo.NV_SHAPE
    _per_row((N, S, E, bo.V, 1.0, 0.3, bo.HOT_NV, hot), f"BCE hot run {hot} E={E}")


@pytest.mark.parametrize("E", bo.WIDTHS)
@pytest.mark.parametrize("nv", bo.NV_TWICE)
def test_chosen_nv_bit_identical(nv, E):
    case = bo.make_case(bo.NV_TWICE_N, bo.NV_SHAPE[1], E, bo.V, 1.0, nv)
    for x, z in zip(_run(*case, beta=0.3), _run(*case, beta=0.3)):
        assert torch.equal(x, z)
