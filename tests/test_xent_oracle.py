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


# ------------------------------------------------ cases with a chosen n_valid
def _all_e16_cases():
    out = [xo.nv_case(xo.NV16_V, N, nv, 16, lay) for nv, N, lay in xo.NV16_CASES]
    out += [xo.edge_case(V, nv, 16) for V in xo.V_EDGES
            for nv in xo.V_EDGE_NV if V <= 5003]
    return out + [xo.family_case(f, 16) for f in xo.FAMILIES]


@pytest.mark.parametrize("layout", xo.LAYOUTS)
@pytest.mark.parametrize("N,nv", [(8, 1), (24, 17), (300, 129), (1030, 129), (64, 64), (5, 0)])
def test_make_nv_case_counts(N, nv, layout):
    """Exactly nv valid tokens, where the layout says, for 0 and -100."""
    for ignore in (0, -100):
        y = xo.make_nv_case(1000, N, nv, 16, layout, ignore=ignore)[3]
        on = torch.nonzero(y != ignore).view(-1)
        assert on.numel() == nv
        assert torch.equal(on, xo.valid_positions(N, nv, layout))
        assert bool(((y[on] >= 0) & (y[on] < 1000)).all())
        if nv == 0:
            continue
        if layout == "front":
            assert int(on[-1]) == nv - 1
        if layout == "back":
            assert int(on[0]) == N - nv
        if layout == "spread" and nv > 1 and N > nv:
            assert int(on[-1]) >= N - 1 - N // nv and int(on[0]) == 0


def test_nv_coverage():
    """The E = 16 list reaches every template instance and threshold."""
    ng0 = {min(8, -(-nv // 16)) for nv, _, _ in xo.NV16_CASES}
    assert ng0 == set(range(1, 9))
    last = {-(-(nv - 128 * ((nv - 1) // 128)) // 16) for nv, _, _ in xo.NV16_CASES if nv > 128}
    assert {1, 8} <= last
    assert {0, 1, 15} <= {nv % 16 for nv, _, _ in xo.NV16_CASES}
    assert {96, 97, 128, 129} <= set(xo.NV16)                  # ring (NG <= 6), fused step
    # valid tokens in the second pass of the compaction loop (index >= 1024, on
    # top of a non-zero base), and valid tokens in front
    assert any(N > 1024 and lay == "back" and N - nv < 1024 for nv, N, lay in xo.NV16_CASES)
    assert any(lay == "front" and N > nv for nv, N, lay in xo.NV16_CASES)
    # V: no ragged tile, only the ragged tile, odd and even counts of full tiles, tpw = 2
    assert any(V % 16 == 0 for V in xo.V_EDGES) and any(V < 16 for V in xo.V_EDGES)
    assert {0, 1} == {(V // 16) % 2 for V in xo.V_EDGES if V >= 16}
    assert any((V + 15) // 16 > 4096 for V in xo.V_EDGES)
    for V in xo.V_EDGES:
        for nv in xo.V_EDGE_NV:
            y = xo.make_nv_case(V, nv + 7, nv, 16, "spread", ignore=xo.edge_ignore(V))[3]
            lab = set(y[y != xo.edge_ignore(V)].tolist())
            assert V - 1 in lab and (V < 16 or 16 * (V // 16 - 1) in lab), V
    # wide: 64-token chunks; mfma: 64-token own tiles
    assert {63, 64, 65} <= set(xo.WIDE_NV) and {63, 64, 65} <= set(xo.MFMA_NV)
    assert {255, 256, 257} <= set(xo.WIDE_V) and {31, 32, 33, 63, 64, 65} <= set(xo.MFMA_V)


def test_families_are_what_they_claim():
    for E in (16, 64, 256):
        H, W, b, y = xo.family_case("hot", E).inputs
        assert torch.unique(y[y != xo.IGNORE]).numel() == 1
        c = xo.family_case("fit", E)
        H, W, b, y = c.inputs
        on = y != xo.IGNORE
        z = H.double() @ W.double().t() + b.double()
        py = torch.softmax(z, 1).gather(1, y.view(-1, 1)).view(-1)[on]
        assert float(py.min()) > 0.999, float(py.min())
        c = xo.family_case("ign100", E)
        y = c.inputs[3]
        assert c.ignore == -100 and int((y == 0).sum()) == 3 and c.nv == xo.FAMILY_SHAPE[2]
        assert xo.family_case("eps0", E).eps == 0.0


def test_yardsticks_finite_and_nonzero():
    """The fp32 reference and the 3-pass emulation have a finite, non-zero
    row_err on every E = 16 case (V = 70001 is left to the GPU run)."""
    for c in _all_e16_cases():
        for kind in ("f32", "x3"):
            for k, v in xo.ref_err(c, kind).items():
                assert 0 < v < 1e-2, (kind, k, v, c.nv)


@pytest.mark.parametrize("E", (32, 64, 128, 256))
def test_fp32_yardstick_wide(E):
    nvs, Vs = (xo.WIDE_NV, xo.WIDE_V) if E <= 64 else (xo.MFMA_NV, xo.MFMA_V)
    for V in Vs:
        for nv in nvs:
            for k, v in xo.ref_err(xo.edge_case(V, nv, E)).items():
                assert 0 < v < 1e-2, (E, V, nv, k, v)


def test_emulation_really_splits():
    """Without the lo terms the emulation is plain bf16: far worse."""
    for nv in (17, 129):
        c = xo.nv_case(xo.NV16_V, nv + 7, nv, 16)
        full = xo.ref_err(c, "x3")
        bare = xo.errs(dict(zip(xo.NAMES5, xo.emulate_x3(*c.inputs, c.eps, c.ignore, lo=False))),
                       c.exact)
        print(f"nv={nv} with lo: {full}\n      without: {bare}")
        for k in ("dH", "loss", "dW", "db"):
            assert bare[k] > 20 * full[k], (k, bare[k], full[k])
        # and it is no better than exact fp32 on the products it replaces
        assert full["dW"] > xo.ref_err(c, "f32")["dW"]


@pytest.mark.parametrize("V,N,nv,E,kw", [(50, 9, 5, 16, {}), (130, 40, 33, 64, dict(eps=0.0)),
                                         (37, 20, 7, 128, dict(ignore=-100))])
def test_nv_oracle_matches_autograd_fp64(V, N, nv, E, kw):
    c = xo.nv_case(V, N, nv, E, "spread", **kw)
    H, W, b, y = c.inputs
    Hd, Wd, bd = (t.double().requires_grad_(True) for t in (H, W, b))
    per = torch.nn.functional.cross_entropy(Hd @ Wd.t() + bd, y, ignore_index=c.ignore,
                                            label_smoothing=c.eps, reduction="none")
    m = per.sum() / nv
    m.backward()
    want = dict(dH=Hd.grad, loss=per.detach(), dW=Wd.grad, db=bd.grad, mean=m.detach())
    for k, r in want.items():
        assert xo.rel_err(c.exact[k], r) < 1e-12, k


def test_db_err_is_row_err_unless_db_cancels():
    """``db_err`` changes the denominator only of elements that lost more
    than the factor 8 to cancellation: never above the plain per-element
    row_err, equal to it where no element cancels that far (V = 3), and below
    it where every row of W expects a label (V = 32 against nv = 129)."""
    from tests import encoder_oracle as eo

    for V, E, same in ((3, 16, True), (32, 256, False)):
        c = xo.edge_case(V, 129, E)
        db, t = c.exact["db"], c.exact["db_terms"]
        assert bool((t >= db.abs() * (1 - 1e-12)).all())
        kappa = float((t / torch.clamp_min(db.abs(), 1e-3 * float(db.abs().max()))).max())
        got = xo.ref_run(c)["db"]
        a, r = xo.db_err(got, db, t), eo.row_err(got, db, "elem")
        print(f"V={V} E={E}: cancellation {kappa:.1f}, db_err {a:.2e}, row_err {r:.2e}")
        assert a <= r and (kappa <= eo.FACTOR) == same and (a == r or not same)
