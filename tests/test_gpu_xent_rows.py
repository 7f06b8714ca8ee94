"""Candidate-subset Linear + label-smoothed CE (csrc/kernels/linear_xent_rows.hip:
sampled softmax), its id sampler and the candidate builder on MI355X, against
the float64 oracles of tests/xent_rows_oracle.py and tests/xent_oracle.py."""
import pytest
import torch

from tdfo_amd import ops
from tests import xent_oracle as xo
from tests import xent_rows_oracle as xr

pytestmark = pytest.mark.gpu
DEV = "cuda"
FILL = 1.0


@pytest.fixture(scope="module", autouse=True)
def _native():
    from tdfo_amd.ops import _ext

    assert _ext.load(), "native library must load on the GPU box"


def _run(H, W, b, cand, target, corr=None, eps=xr.EPS):
    """ops.linear_xent_rows on device copies -> [dH, lossv, dW, db, loss];
    dW / db are pre-filled with FILL."""
    N, E = H.shape
    V = W.shape[0]
    out = [torch.zeros(N, E, device=DEV), torch.zeros(N, device=DEV),
           torch.full((V, E), FILL, device=DEV), torch.full((V,), FILL, device=DEV)]
    loss = torch.zeros(1, device=DEV)
    ops.linear_xent_rows(H.to(DEV), W.to(DEV), b.to(DEV), cand.to(DEV), target.to(DEV), eps, *out,
                         loss=loss, corr=None if corr is None else corr.to(DEV))
    torch.cuda.synchronize()
    return out + [loss]


def _check(out, want, cand, V, tag):
    """Every output within BOUND of fp64 on the rows the call owns; every
    other row of dW / db still holds its fill, exactly."""
    rows = cand[xr.valid_slots(cand, V)]
    named = torch.zeros(V, dtype=torch.bool)
    named[rows] = True
    dW, db = out[2].cpu(), out[3].cpu()
    assert bool((dW[~named] == FILL).all()) and bool((db[~named] == FILL).all()), tag
    got = [out[0], out[1], dW[named], db[named], out[4][0]]
    ref = [want[0], want[1], want[2][named], want[3][named], want[4]]
    errs = {k: xo.rel_err(a, r) for k, a, r in zip(xr.NAMES, got, ref)}
    print(f"kernel vs fp64 {tag}: " + " ".join(f"{k}={v:.2e}" for k, v in errs.items()))
    for k, v in errs.items():
        assert v < xr.BOUND, (tag, k, v)


def _check_one_candidate(out, case, tag):
    """Mv = 1: the softmax is 1 = eps / 1 + (1 - eps), so every output is an
    exact cancellation to 0 and rel_err's denominator (the result's magnitude)
    vanishes. The error is measured against the magnitude of the terms that
    cancel instead, with the same BOUND: |W_y| / nv for dH, |H| / nv for dW,
    1 / nv for db, |z| for the per-token and the mean loss."""
    H, W, b, cand, target, _ = case
    V = W.shape[0]
    row = int(cand[0])
    nv = int((target == 0).sum())
    z = float((H.double() @ W[row].double() + b[row].double()).abs().max())
    named = torch.zeros(V, dtype=torch.bool)
    named[row] = True
    dW, db = out[2].cpu(), out[3].cpu()
    assert bool((dW[~named] == FILL).all()) and bool((db[~named] == FILL).all()), tag
    scale = {"dH": float(W[row].abs().max()) / nv, "loss": z, "dW": float(H.abs().max()) / nv,
             "db": 1.0 / nv, "mean": z}
    got = {"dH": out[0], "loss": out[1], "dW": dW[named], "db": db[named], "mean": out[4]}
    errs = {k: float(got[k].abs().max()) / scale[k] for k in xr.NAMES}
    print(f"kernel vs 0 {tag}: " + " ".join(f"{k}={v:.2e}" for k, v in errs.items()))
    for k, v in errs.items():
        assert v < xr.BOUND, (tag, k, v)


@pytest.mark.parametrize("E", xr.WIDTHS)
def test_kernel_matches_fp64_oracle(E):
    """dH, per-token loss, dW, db and the mean loss within 2e-4 of fp64 at
    every shape, with H scaled by 12, with a corr, and at a larger V."""
    cases = [(N, M, xr.V, 1.0, False) for N, M in xr.SHAPES]
    cases += [(320, 513, xr.V, 12.0, False), (320, 129, xr.V, 1.0, True),
              (65, 65, 70001, 1.0, False)]
    for N, M, V, hs, wc in cases:
        case = xr.make_case(N, M, E, V, hs, wc)
        out = _run(*case)
        tag = f"N={N} M={M} V={V} hs={hs} corr={wc} E={E}"
        if M == 1:
            _check_one_candidate(out, case, tag)
        else:
            _check(out, xr.oracle_case(N, M, E, V, hs, wc), case[3], V, tag)


@pytest.mark.parametrize("E", xr.WIDTHS)
def test_equals_full_softmax(E):
    """cand = arange(V) (and a random permutation of it, targets remapped) is
    the full softmax: within BOUND of its own oracle."""
    V, N = 1000, 320
    H, W, b, y = xo.make_case(V, N, 1.0, E)
    want = xo.oracle_case(V, N, 1.0, E)
    ident = torch.arange(V)
    g = torch.Generator().manual_seed(E)
    perm = torch.randperm(V, generator=g)
    inv = torch.empty_like(perm)
    inv[perm] = torch.arange(V)
    for name, cand, slot in (("arange", ident, ident), ("permuted", perm, inv)):
        target = torch.where(y == xo.IGNORE, -torch.ones_like(y), slot[y])
        out = _run(H, W, b, cand, target, eps=xo.EPS)
        out[4] = out[4][0]
        errs = {k: xo.rel_err(a, r) for k, a, r in zip(xr.NAMES, out, want)}
        print(f"vs the full softmax's oracle, {name}, E={E}: "
              + " ".join(f"{k}={v:.2e}" for k, v in errs.items()))
        for k, v in errs.items():
            assert v < xr.BOUND, (name, k, v)


@pytest.mark.parametrize("E", xr.WIDTHS)
def test_holes_are_free(E):
    """A call with holes equals, bit for bit, the call with the holes removed
    and the targets remapped; two identical calls are bit-identical."""
    for N, M in [(320, 513), (65, 64)]:
        H, W, b, cand, target, corr = xr.make_case(N, M, E, xr.V, 1.0, True)
        a = _run(H, W, b, cand, target, corr)
        a2 = _run(H, W, b, cand, target, corr)
        c2, t2, r2 = xr.without_holes(cand, target, xr.V, corr)
        assert c2.numel() < M
        c = _run(H, W, b, c2, t2, r2)
        for x, y, z in zip(a, a2, c):
            assert torch.equal(x, y), (N, M)
            assert torch.equal(x, z), (N, M)


@pytest.mark.parametrize("E", xr.WIDTHS)
def test_forced_splits(E):
    """Forced candidate splits 1, 2, 3, 7 are each within the bound, and the
    hook restores."""
    N, M = 320, 513
    case = xr.make_case(N, M, E)
    want = xr.oracle_case(N, M, E)
    before = ops.linear_xent_splits(-1)
    try:
        for n in (1, 2, 3, 7):
            prev = ops.linear_xent_splits(n)
            assert ops.linear_xent_splits(-1) == n
            _check(_run(*case), want, case[3], xr.V, f"N={N} M={M} E={E} splits={n}")
            assert ops.linear_xent_splits(prev) == n
    finally:
        ops.linear_xent_splits(before)
    assert ops.linear_xent_splits(-1) == before


@pytest.mark.parametrize("E", xr.WIDTHS)
def test_nothing_valid(E):
    """All tokens ignored, all candidates holes, and every target on a hole:
    zero dH / lossv / loss, and nothing written to dW / db."""
    N, M, V = 65, 70, 300
    g = torch.Generator().manual_seed(E)
    H, W = torch.randn(N, E, generator=g), torch.randn(V, E, generator=g)
    b = torch.randn(V, generator=g)
    cand = torch.randperm(V, generator=g)[:M]
    holes = torch.full((M,), -1, dtype=torch.int64)
    half = cand.clone()
    half[::2] = V + 1
    on_hole = torch.zeros(N, dtype=torch.int64) + 2 * torch.arange(N).remainder(M // 2)
    for name, c, t in (("tokens ignored", cand, torch.full((N,), -1, dtype=torch.int64)),
                       ("candidates holes", holes, torch.arange(N).remainder(M)),
                       ("targets on holes", half, on_hole)):
        dH, lv = torch.ones(N, E, device=DEV), torch.ones(N, device=DEV)
        dW, db = torch.full((V, E), FILL, device=DEV), torch.full((V,), FILL, device=DEV)
        loss = torch.ones(1, device=DEV)
        ops.linear_xent_rows(H.to(DEV), W.to(DEV), b.to(DEV), c.to(DEV), t.to(DEV), 0.1, dH, lv,
                             dW, db, loss=loss)
        torch.cuda.synchronize()
        assert float(dH.abs().sum()) == 0 and float(lv.abs().sum()) == 0, name
        assert float(loss) == 0, name
        assert bool((dW == FILL).all()) and bool((db == FILL).all()), name


@pytest.mark.parametrize("E", xr.WIDTHS)
def test_empty_launches_nothing(E):
    """N = 0 and M = 0: nothing is launched and the outputs keep their fill."""
    V = 100
    W, b = torch.randn(V, E, device=DEV), torch.zeros(V, device=DEV)
    i64 = dict(dtype=torch.int64, device=DEV)
    for N, M in ((0, 5), (7, 0)):
        dH, lv = torch.full((N, E), 3.0, device=DEV), torch.full((N,), 3.0, device=DEV)
        dW, db = torch.full((V, E), FILL, device=DEV), torch.full((V,), FILL, device=DEV)
        loss = torch.full((1,), 5.0, device=DEV)
        ops.linear_xent_rows(torch.randn(N, E, device=DEV), W, b, torch.arange(M, **i64),
                             torch.zeros(N, **i64), 0.1, dH, lv, dW, db, loss=loss)
        torch.cuda.synchronize()
        assert bool((dH == 3).all()) and bool((lv == 3).all())
        assert bool((dW == FILL).all()) and bool((db == FILL).all()) and float(loss) == 5.0


def test_host_side_width_check():
    """An unsupported width raises on the host naming the supported set,
    nothing is written, and a valid call afterwards passes."""
    V, N, M, E = 50, 7, 9, 96
    dH, lv = torch.ones(N, E, device=DEV), torch.ones(N, device=DEV)
    dW, db = torch.ones(V, E, device=DEV), torch.ones(V, device=DEV)
    i64 = dict(dtype=torch.int64, device=DEV)
    with pytest.raises(RuntimeError, match=r"16\|32\|64\|128\|256"):
        ops.linear_xent_rows(torch.randn(N, E, device=DEV), torch.randn(V, E, device=DEV),
                             torch.zeros(V, device=DEV), torch.arange(M, **i64),
                             torch.zeros(N, **i64), 0.1, dH, lv, dW, db)
    torch.cuda.synchronize()
    for t in (dH, lv, dW, db):
        assert bool((t == 1).all())
    case = xr.make_case(7, 7, 64)
    _check(_run(*case), xr.oracle_case(7, 7, 64), case[3], xr.V, "after a refused call")


def test_no_logits_in_hbm():
    """The call's peak allocation stays under a quarter of an [N, M] fp32
    tensor (dW / db are the caller's)."""
    N, M, V, E = 512, 20000, 200_000, 64
    g = torch.Generator().manual_seed(5)
    H = torch.randn(N, E, generator=g).to(DEV)
    W = (torch.randn(V, E, generator=g) * 0.2).to(DEV)
    b = torch.zeros(V, device=DEV)
    cand = torch.randperm(V, generator=g)[:M].to(DEV)
    target = torch.randint(0, M, (N,), generator=g).to(DEV)
    out = [torch.zeros(N, E, device=DEV), torch.zeros(N, device=DEV),
           torch.zeros(V, E, device=DEV), torch.zeros(V, device=DEV)]
    ops.linear_xent_rows(H, W, b, cand, target, 0.1, *out)              # warm-up
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.max_memory_allocated()
    ops.linear_xent_rows(H, W, b, cand, target, 0.1, *out)
    torch.cuda.synchronize()
    grew = torch.cuda.max_memory_allocated() - base
    print(f"peak allocation across the call: {grew} bytes; logits would be {N * M * 4}")
    assert grew < N * M * 4 // 4
    assert bool(torch.isfinite(out[1]).all()) and float(out[1].min()) > 0


def test_sampler_matches_mirror():
    """The GPU sampler equals the Python mirror bit for bit, stays in
    [lo, hi), and draws a different vector at the next step."""
    n, lo, hi = 5000, 1, 300_001
    for seed, step in ((42, 0), (42, 1), (7, 123456)):
        st = torch.tensor([step], dtype=torch.int64)
        want = torch.empty(n, dtype=torch.int64)
        ops.sample_ids(seed, st, lo, hi, want)
        got = torch.empty(n, dtype=torch.int64, device=DEV)
        ops.sample_ids(seed, st.to(DEV), lo, hi, got)
        nxt = torch.empty(n, dtype=torch.int64, device=DEV)
        ops.sample_ids(seed, (st + 1).to(DEV), lo, hi, nxt)
        assert torch.equal(got.cpu(), want), (seed, step)
        assert int(got.min()) >= lo and int(got.max()) < hi
        assert not torch.equal(got, nxt)


def test_candidate_builder():
    """N = 1030, S = 512, repeated negatives and a negative equal to a label:
    the valid candidates are distinct and are the union, and every
    non-ignored token's target names its label."""
    labels, neg = xr.candidate_case()
    cand = torch.zeros(labels.numel() + neg.numel(), dtype=torch.int64, device=DEV)
    target = torch.zeros(labels.numel(), dtype=torch.int64, device=DEV)
    ops.xent_candidates(labels.to(DEV), neg.to(DEV), 0, cand, target)
    torch.cuda.synchronize()
    xr.check_candidates(labels, neg, cand, target)


# --------------------------------------------- per row, at chosen valid counts
@pytest.mark.parametrize("E", xr.WIDTHS)
@pytest.mark.parametrize("nv", xr.NV)
def test_chosen_nv_per_row(nv, E):
    """Exactly nv valid tokens (the 64-token own tile at its edges): dH and
    dW per row, lossv and db per element and the mean within
    max(8 x row_err(fp32 reference), 2^-20) of fp64; the rows no candidate
    names keep their fill; ignored tokens get exact zeros."""
    N, M = xr.NV_SHAPE
    args = (N, M, E, xr.V, 1.0, False, nv)
    case = xr.make_case(*args)
    out = _run(*case)
    named = xr.named_rows(case[3], xr.V)
    assert bool((out[2].cpu()[~named] == FILL).all()) and bool((out[3].cpu()[~named] == FILL).all())
    xr.assert_within(out[:4] + [out[4][0]], args, f"rows CE E={E} N={N} M={M} nv={nv}")
    want = xr.oracle_case(*args)
    ign = want[1] == 0
    assert int((~ign).sum()) == nv
    assert float(out[0].cpu()[ign].abs().sum()) == 0 and float(out[1].cpu()[ign].abs().sum()) == 0


@pytest.mark.parametrize("E", xr.WIDTHS)
@pytest.mark.parametrize("nv", xr.NV_TWICE)
def test_chosen_nv_bit_identical(nv, E):
    case = xr.make_case(xr.NV_TWICE_N, xr.NV_SHAPE[1], E, xr.V, 1.0, False, nv)
    for x, z in zip(_run(*case), _run(*case)):
        assert torch.equal(x, z)
