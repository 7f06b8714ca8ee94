"""CPU self-check of tests/tail_oracle.py: every case of the GPU file through
``ops.*`` on CPU tensors (the fp32 reference) and through the same check
functions, and the teeth tests -- each hands a deliberately wrong result to
the shared check, which must reject it for the stated reason."""
import pytest
import torch

from tdfo_amd import ops
from tdfo_amd.ops import _ext
from tests import tail_oracle as to
from tests.tail_oracle import BF, F32, body

CPU = "cpu"


def test_case_lists_skip_nothing():
    """no case list is empty, holds duplicates or loses a value the sweep names"""
    for name, cases in to.CASE_LISTS.items():
        assert len(cases) > 0 and len(set(cases)) == len(cases), name
    assert {(c.K, c.B, c.relu) for c in to.HEAD_CASES if not c.sat and not c.frac} == \
        {(K, B, r) for K in (16, 32, 64, 128, 256, 512, 1024) for B in (1, 15, 16, 17, 37)
         for r in (True, False)}
    assert {c.K for c in to.HEAD_CASES if c.sat} == set(to.HEAD_KS)
    assert any(c.frac for c in to.HEAD_CASES)
    assert {c.n for c in to.RR_CASES} == {1, 15, 16, 17, 16383, 16384, 16384 + 65, 8192 * 64 + 67}
    assert {c.rows for c in to.RR_CASES if c.PH == 16} >= {1, 3, 63, 64, 65, 77}
    assert {c.rows for c in to.RR_CASES if c.PH == 4} >= {1, 3, 15, 16, 17, 77}
    assert {(c.acc, round(c.scale, 3)) for c in to.RR_CASES} == \
        {(a, s) for a in (False, True) for s in (1.0, 0.5, 0.333)}
    assert len(to.CS_CASES) == 5 * 4 * 2
    assert {(c.opt, c.step, c.wd, c.gs, c.n) for c in to.DO_CASES if c.found is None} >= \
        {(o, t, w, g, n) for o in to.DO_OPTS for t in (1.0, 2.0, 5.0, 1e6) for w in (0.0, 0.01)
         for g in (1.0, 0.5) for n in (4, 4160)}
    assert any(c.n == 4096 * 256 * 4 + 1028 for c in to.DO_CASES)
    assert {c.bf16 for c in to.DO_CASES} == {True, False}
    assert len(to.CF_CASES) == 6 * 9 + 6 * 2 + 1
    assert {(c.nb, c.n) for c in to.AH_CASES if c.kind == "interior"} == \
        {(nb, n) for nb in (1, 2, 199, 200, 512, 2048) for n in (1, 255, 256, 257, 1024 * 256 + 3)}
    assert {c.nparts for c in to.RA_CASES} == {1, 15, 16, 17, 63, 64, 65, 511, 512, 513, 600}
    assert {c.n for c in to.RA_CASES} == {15, 16, 2400}
    assert {(c.nb, c.nlog) for c in to.RA_CASES} >= {(0, 0), (199, 1), (199, 1000), (512, 1),
                                                      (512, 1000)}
    assert {c.adamw for c in to.RA_CASES} == {True, False}
    assert len(to.GLUE_CASES) == 8 and len(to.CROSS_CASES) == 8 and len(to.BL_CASES) == 12


# ------------------------------------------------------------------ head_bce
@pytest.mark.parametrize("case", to.HEAD_CASES, ids=to.head_id)
def test_head_bce(case):
    got = to.run_head(case, CPU)
    to.check_head(case, got, to.head_yard(case))
    to.check_head_chain(case, got, CPU)


def test_head_oracle_matches_autograd():
    """the hand-written float64 backward against torch.autograd"""
    c = to.HeadCase(64, 17, True)
    d = to.head_data(c)
    H = d["H"].clone().requires_grad_(True)
    w = d["w"].clone().requires_grad_(True)
    b = d["b"].clone().requires_grad_(True)
    x = H @ w + b
    loss = torch.nn.functional.binary_cross_entropy_with_logits(x, d["y"], reduction="sum")
    (loss * d["inv_n"]).backward()
    e = to.head_exact(c, d["x"])
    assert torch.allclose(e["dw"], w.grad, rtol=1e-12, atol=1e-15)
    assert torch.allclose(e["db"], b.grad[0], rtol=1e-12, atol=1e-15)
    assert torch.allclose(e["dH"], torch.where(e["live"], H.grad, torch.zeros_like(H)),
                          rtol=1e-12, atol=1e-15)
    assert abs(float(e["loss"]) - float(loss)) < 1e-12 * float(loss)


TEETH_HEAD = to.HeadCase(64, 17, True)            # B = 17: a block with one sample
TEETH_SAT = to.HeadCase(64, 37, True, sat=True)


def _head_got(c):
    return {k: v.clone() for k, v in to.run_head(c, CPU).items()}


def test_teeth_dh_unmasked_at_negative_zero():
    c = TEETH_HEAD
    d, got = to.head_data(c), _head_got(c)
    H = d["H"]
    s, k = ((H == 0) & torch.signbit(H)).nonzero()[0].tolist()
    g = to.head_exact(c, d["x"])["g"]
    body_ = to._dh_slot(c, BF).view(got["dH"])
    body_[s, k] = float(g[s] * d["w"][k])
    assert float(body_[s, k]) != 0
    with pytest.raises(AssertionError, match="masked element is not exactly 0"):
        to.check_head(c, got, to.head_yard(c))


def test_teeth_dh_column_of_another_sample():
    c = TEETH_HEAD
    d, got = to.head_data(c), _head_got(c)
    e = to.head_exact(c, d["x"])
    k = int(d["w"].abs().argmax())
    live = e["live"][:, k].nonzero().view(-1)
    s = int(live[0])
    t = int(live[(e["g"][live] - e["g"][s]).abs().argmax()])
    to._dh_slot(c, BF).view(got["dH"])[s, k] = float(e["dH"][t, k])
    with pytest.raises(AssertionError, match="head_bce dH: outside its bound"):
        to.check_head(c, got, to.head_yard(c))


def test_teeth_dw_misses_last_sample_of_partial_block():
    c = TEETH_HEAD
    d, got = to.head_data(c), _head_got(c)
    e = to.head_exact(c, d["x"])
    part = d["slots"]["part"].view(got["part"]).view(d["nparts"], c.K + 2)
    part[0, :c.K] -= (e["g"][-1] * d["H"][-1]).float()
    with pytest.raises(AssertionError, match="head_bce dw: outside its bound"):
        to.check_head(c, got, to.head_yard(c))


def test_teeth_loss_without_max_term_at_saturated_logit():
    c = TEETH_SAT
    d, got = to.head_data(c), _head_got(c)
    x, y = d["x"], d["y"]
    wrong = (-x * y + torch.log1p(torch.exp(-x.abs()))).sum()      # no max(x, 0)
    assert float(x.clamp_min(0).sum()) > 50
    part = d["slots"]["part"].view(got["part"]).view(d["nparts"], c.K + 2)
    part[:, c.K + 1] = 0
    part[0, c.K + 1] = float(wrong)
    with pytest.raises(AssertionError, match="head_bce loss: outside its bound"):
        to.check_head(c, got, to.head_yard(c))


def test_teeth_output_element_left_unwritten():
    c = TEETH_HEAD
    got = _head_got(c)
    to.head_data(c)["slots"]["logits"].view(got["logits"])[c.B - 1] = float("nan")
    with pytest.raises(AssertionError, match="logits: an element was never written"):
        to.check_head(c, got, to.head_yard(c))


def test_teeth_write_into_a_ring():
    c = TEETH_HEAD
    got = _head_got(c)
    s = to._dh_slot(c, BF)
    got["dH"][s.off + c.K] = 0.0                     # the column after row 0's last
    with pytest.raises(AssertionError, match="head_bce dH: written outside its view"):
        to.check_head(c, got, to.head_yard(c))
    got = _head_got(c)
    got["part"][to.head_data(c)["slots"]["part"].off - 1] = 0.0
    with pytest.raises(AssertionError, match="head_bce part: written outside its view"):
        to.check_head(c, got, to.head_yard(c))


# --------------------------------------------------------------- reductions
@pytest.mark.parametrize("mode", ["exact", "float"])
@pytest.mark.parametrize("case", to.RR_CASES, ids=to.rr_id)
def test_reduce_rows(case, mode):
    to.check_rr(case, mode, to.run_rr(case, mode, CPU), bitwise=False)


@pytest.mark.parametrize("PH,rows", [(16, 65), (16, 600), (4, 17), (16, 3)])
def test_fixed_order_is_a_permutation_of_the_rows(PH, rows):
    """the documented order adds every row exactly once (integer data: any
    order gives the plain sum)"""
    p = torch.randint(-8, 9, (rows, 5), generator=to._gen(1, PH, rows)).float()
    assert torch.equal(to.fixed_order_column_sums(p, PH), p.sum(0))


def test_fma_f32_rounds_once():
    """fma_f32 against exact rational arithmetic; the scales make the exact
    sum longer than float64's 53 bits in three quarters of the elements"""
    from fractions import Fraction

    import numpy as np

    def exact(a, b, c):
        v = Fraction(float(a)) * Fraction(float(b)) + Fraction(float(c))
        lo = np.float32(float(v))                          # a neighbour of the answer
        cands = [np.nextafter(lo, np.float32(-np.inf)), lo, np.nextafter(lo, np.float32(np.inf))]
        best = min(cands, key=lambda f: (abs(Fraction(float(f)) - v), int(f.view(np.uint32)) & 1))
        return float(best)

    g = to._gen(7)
    a = torch.randn(400, generator=g)
    c = torch.randn(400, generator=g) * torch.tensor([1.0, 1e-3, 1e3, 1e-7]).repeat(100)
    b = to.f32(1 / 3)
    got = to.fma_f32(a, b, c)
    want = torch.tensor([exact(x, b, y) for x, y in zip(a.tolist(), c.tolist())])
    assert torch.equal(got, want)


TEETH_RR = to.RRCase(17, 65, True, 0.5)


def test_teeth_reduce_rows_fma_case_accepts_two_patterns_only():
    c = to.RRCase(17, 65, True, 1 / 3)
    assert c in to.RR_CASES
    d = to.rr_data(c, "float")
    fo = to.fixed_order_column_sums(d["p"], 16)
    for ok in ((d["o0"].double() + (fo.double() * to.f32(1 / 3)).float().double()).float(),
               to.fma_f32(fo, to.f32(1 / 3), d["o0"])):
        to.check_rr(c, "float", to.fresh(d["os"], CPU, init=ok), bitwise=True)
    off = torch.nextafter(ok, torch.full_like(ok, 9.0))        # one ulp off
    with pytest.raises(AssertionError, match="bits differ from the unfused and the fused"):
        to.check_rr(c, "float", to.fresh(d["os"], CPU, init=off), bitwise=True)


def test_teeth_reduce_rows_drops_partial_last_group():
    c = TEETH_RR
    d = to.rr_data(c, "exact")
    got = to.run_rr(c, "exact", CPU).clone()
    # rows 64.. are the partial last group of phase 0
    d["os"].view(got).copy_(d["o0"] + 0.5 * d["p"][:64].sum(0))
    assert float(d["p"][64].abs().sum()) > 0
    with pytest.raises(AssertionError, match="reduce_rows out: bits differ"):
        to.check_rr(c, "exact", got, bitwise=True)


def test_teeth_reduce_rows_scales_before_accumulating():
    c = TEETH_RR
    d = to.rr_data(c, "float")
    got = to.run_rr(c, "float", CPU).clone()
    d["os"].view(got).copy_((d["o0"] + d["p"].sum(0)) * 0.5)       # scale applied to out too
    with pytest.raises(AssertionError, match="reduce_rows out: outside its bound"):
        to.check_rr(c, "float", got, bitwise=False)


@pytest.mark.parametrize("mode", ["exact", "float"])
@pytest.mark.parametrize("case", to.CS_CASES, ids=to.cs_id)
def test_colsum(case, mode):
    to.check_cs(case, mode, to.run_cs(case, mode, CPU))


def test_teeth_colsum_drops_last_row_chunk():
    c = to.CSCase(533, 72, False)
    d = to.cs_data(c, "exact")
    got = to.run_cs(c, "exact", CPU).clone()
    per = -(-c.M // 16)                                  # rows of one of the 16 chunks
    d["os"].view(got).copy_(d["x"][:15 * per].sum(0))
    with pytest.raises(AssertionError, match="colsum out"):
        to.check_cs(c, "exact", got)


# ---------------------------------------------------------- dense optimizer
@pytest.mark.parametrize("case", to.DO_CASES, ids=to.do_id)
def test_dense_optimizer(case):
    to.check_do(case, to.run_do(case, CPU), to.do_yard(case), float)


@pytest.mark.parametrize("mode", ["exact", "float"])
def test_dense_optimizer_slab_segments(mode):
    to.check_slab(mode, to.run_slab(mode, CPU))


@pytest.mark.parametrize("opt", to.DO_OPTS)
def test_dense_optimizer_found_inf_zero_equals_unflagged(opt):
    to.check_do_flag_zero(opt, CPU)


def _do_wrong(c, **over):
    """the reference's outputs with p (and m) replaced by a wrong formula"""
    d = to.do_data(c)
    got = {k: v.clone() for k, v in to.run_do(c, CPU).items()}
    for k, v in over.items():
        d["slots"][k].view(got[k]).copy_(v)
    if "p" in over and c.bf16 and "pb" not in over:
        d["slots"]["pb"].view(got["pb"]).copy_(body(d["slots"]["p"], got["p"]).to(BF))
    return got


def _adam_parts(c):
    d = to.do_data(c)
    p, g, m, v = (d[k].double() for k in ("p", "g", "m", "v"))
    b1, b2, eps, lr = to.B1, to.B2, to.EPS, to.f32(to.LR)
    gg = g * to.f32(c.gs)
    p1 = p - lr * c.wd * p
    m1, v1 = b1 * m + (1 - b1) * gg, b2 * v + (1 - b2) * gg * gg
    return p1, m1, v1, b1, b2, eps, lr


TEETH_ADAM = to.DOCase("adamw", 2.0, 0.01, 0.5, 4160, bf16=True, found=0.0)
assert TEETH_ADAM in to.DO_CASES


def test_teeth_adam_eps_inside_sqrt():
    c = TEETH_ADAM
    p1, m1, v1, b1, b2, eps, lr = _adam_parts(c)
    wrong = p1 - lr * (m1 / (1 - b1 ** c.step)) / (v1 / (1 - b2 ** c.step) + eps).sqrt()
    with pytest.raises(AssertionError, match="dense_optimizer p: outside its bound") as ei:
        to.check_do(c, _do_wrong(c, p=wrong), to.do_yard(c), float)
    assert ei.value.args[0][2][0] in (1, 2)          # the planted v = 0 / v ~ 1e-16 elements


def test_teeth_adam_bc2_at_previous_step():
    c = TEETH_ADAM
    p1, m1, v1, b1, b2, eps, lr = _adam_parts(c)
    wrong = p1 - lr * (m1 / (1 - b1 ** c.step)) / ((v1 / (1 - b2 ** (c.step - 1))).sqrt() + eps)
    with pytest.raises(AssertionError, match="dense_optimizer p: outside its bound"):
        to.check_do(c, _do_wrong(c, p=wrong), to.do_yard(c), float)


def test_teeth_sgd_momentum_multiplies_m_on_step_one():
    c = to.DOCase("sgd", 1.0, 0.0, 1.0, 4160, bf16=True)
    assert c in to.DO_CASES
    d = to.do_data(c)
    p, g, m = (d[k].double() for k in ("p", "g", "m"))
    m1 = to.MOM * m + g
    with pytest.raises(AssertionError, match="dense_optimizer m: outside its bound"):
        to.check_do(c, _do_wrong(c, p=p - to.f32(to.LR) * m1, m=m1), 0.0, float)


def test_teeth_p_bf16_truncated():
    c = TEETH_ADAM
    d = to.do_data(c)
    got = {k: v.clone() for k, v in to.run_do(c, CPU).items()}
    p = body(d["slots"]["p"], got["p"])
    trunc = (p.view(torch.int32) & -65536).view(F32).to(BF)
    assert not torch.equal(trunc, p.to(BF))
    d["slots"]["pb"].view(got["pb"]).copy_(trunc)
    with pytest.raises(AssertionError, match="p_bf16: not the round-to-nearest-even bf16"):
        to.check_do(c, got, to.do_yard(c), float)


def test_teeth_found_inf_ignored():
    c = to.DOCase("adamw", 2.0, 0.01, 0.5, 4160, bf16=True, found=1.0)
    assert c in to.DO_CASES
    stepped = to.run_do(to.DOCase("adamw", 2.0, 0.01, 0.5, 4160, bf16=True, found=0.0), CPU)
    got = {k: v.clone() for k, v in to.run_do(c, CPU).items()}
    for k in ("p", "m", "v", "pb"):
        got[k] = stepped[k].clone()
    with pytest.raises(AssertionError, match="dense_optimizer p under found_inf: bits differ"):
        to.check_do(c, got, 0.0)


# ------------------------------------------------- check_finite, cast_bf16
@pytest.mark.parametrize("case", to.CF_CASES, ids=to.cf_id)
def test_check_finite(case):
    to.check_cf(case, to.run_cf(case, CPU))


def test_teeth_check_finite_clears_flag():
    case = (4099, None, None, 1.0)
    assert case in to.CF_CASES
    got = to.run_cf(case, CPU).clone()
    to.vec_slot(1, F32).view(got).fill_(0.0)
    with pytest.raises(AssertionError, match="only ever set"):
        to.check_cf(case, got)


@pytest.mark.parametrize("n", to.CAST_NS)
def test_cast_bf16(n):
    to.check_cast(n, to.run_cast(n, CPU))


def test_rne_bits_by_hand():
    """the integer rounding on values worked out by hand"""
    import numpy as np
    x = torch.tensor(np.array([0x3F808000, 0x3F818000, 0x7F7FFFFF, 0x7F800001, 0x80000000,
                               0x00008000, 0x00018000, 0x3F808001], dtype=np.uint32).view(np.float32))
    assert to.rne_bits(x).tolist() == [0x3F80, 0x3F82, 0x7F80, -1, 0x8000, 0, 2, 0x3F81]


# ----------------------------------------------------------------- auc_hist
@pytest.mark.parametrize("case", to.AH_CASES, ids=to.ah_id)
def test_auc_hist(case):
    to.check_ah(case, to.run_ah(case, CPU))


TEETH_AH = to.AHCase(200, 257)


def test_teeth_hist_classes_swapped():
    c = TEETH_AH
    d = to.ah_data(c)
    got = to.run_ah(c, CPU).clone()
    h = d["hs"].view(got)
    delta = (h - d["h0"]).view(2, c.nb)
    h.copy_(d["h0"] + delta.flip(0).reshape(-1))
    with pytest.raises(AssertionError, match="auc_hist: (per-class totals|counts differ)"):
        to.check_ah(c, got)


def test_teeth_hist_label_threshold_inclusive():
    c = TEETH_AH
    d = to.ah_data(c)
    assert float(d["y"][1]) == 0.5
    h = d["h0"].clone()
    ops.auc_hist(d["x"], (d["y"] >= 0.5).float(), c.nb, h)          # 0.5 counted as positive
    got = to.fresh(d["hs"], CPU, init=h)
    with pytest.raises(AssertionError, match="auc_hist: per-class totals"):
        to.check_ah(c, got)


def test_auc_hist_nb_limit_is_refused():
    """the binding refuses a bucket count whose LDS a block cannot have, before
    it looks at the tensors (so the refusal is reachable without a GPU). Needs
    the native library that ``build()`` of __graft_entry__.py leaves in the
    tree; it is not built from here, and its absence or a failed load fails."""
    assert _ext.lib_path().exists(), \
        f"native library {_ext.lib_path()} not built: run build() of __graft_entry__.py first"
    assert _ext.load(build_if_missing=False), "native library failed to load"
    x = torch.zeros(4)
    for nb in (8193, 1 << 20, 0):
        h = torch.zeros(2 * nb, dtype=torch.int64)
        with pytest.raises(RuntimeError, match=r"1 <= nb <= 8192"):
            _ext.ops().auc_hist(x, x, nb, h)
        assert int(h.sum()) == 0


# -------------------------------------------------------------- reduce_adam
@pytest.mark.parametrize("mode", ["exact", "float"])
@pytest.mark.parametrize("case", to.RA_CASES, ids=to.ra_id)
def test_reduce_adam(case, mode):
    got = to.run_ra(case, mode, CPU)
    to.check_ra(case, mode, got, False, to.ra_yard(case, mode), float)
    to.check_ra_same(case, mode, got, to.run_ra(case, mode, CPU, separate=True))


# ------------------------------------------------------ DCN glue, batch_load
@pytest.mark.parametrize("F,D,B", to.GLUE_CASES)
def test_concat_features(F, D, B):
    to.check_concat(F, D, B, to.run_concat(F, D, B, CPU))


@pytest.mark.parametrize("pitched", [False, True])
@pytest.mark.parametrize("relu", [True, False])
@pytest.mark.parametrize("F,D,B", to.GLUE_CASES)
def test_split_features(F, D, B, relu, pitched):
    to.check_split(F, D, B, relu, to.run_split(F, D, B, relu, pitched, CPU))


@pytest.mark.parametrize("mode", ["exact", "float"])
@pytest.mark.parametrize("n,acc,add", to.CROSS_CASES)
def test_cross_bwd(n, acc, add, mode):
    to.check_cross(n, acc, add, mode, to.run_cross(n, acc, add, mode, CPU))


@pytest.mark.parametrize("B,nd,ni", to.BL_CASES)
def test_batch_load(B, nd, ni):
    to.check_bl(B, nd, ni, to.run_bl(B, nd, ni, CPU))
