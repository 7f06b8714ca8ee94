"""The loss head, the deterministic reductions, the flat optimizer, the AUC
histogram and the DCN glue (csrc/kernels/loss.hip, optim.hip, elementwise.hip,
csrc/include/tdfo_reduce_adam.h) against the float64 oracles of
tests/tail_oracle.py: the cases of tests/test_tail_oracle.py through the HIP
kernels. Exact mode -- integer data whose every partial sum is representable,
so results must equal the oracle -- and float mode with per-element bounds:
derived where the arithmetic is IEEE fp32, FACTOR x the fp32 reference's own
error (floored) where an intrinsic is involved. reduce_rows, head_reduce and
reduce_adam must also reproduce their documented summation order bit for bit,
and reduce_adam the separate launches. Operands sit in NaN-filled parents and
outputs in sentinel-filled ones: a clamped or stray read that reaches a
result, a write outside the view and an element never written all fail."""
import pytest
import torch

from tdfo_amd import ops
from tests import tail_oracle as to

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
WORST = {}                       # op -> worst float-mode error / bound
YARD = {}                        # op -> largest reference yardstick it was held to


def _note(op, ratio, yard=None):
    WORST[op] = max(WORST.get(op, 0.0), ratio)
    if yard is not None:
        YARD[op] = max(YARD.get(op, 0.0), yard)


@pytest.fixture(scope="module", autouse=True)
def report_worst_ratios():
    """After the file's tests: the worst float-mode error / bound per op and
    the largest reference yardstick behind a measured bound (shown with -s)."""
    yield
    for op in sorted(WORST):
        tail = f"  (reference yardstick <= {YARD[op]:.3g})" if op in YARD else ""
        print(to.worst_ratio_line(op, WORST[op]) + tail)


@pytest.mark.parametrize("case", to.HEAD_CASES, ids=to.head_id)
def test_head_bce(case):
    got = to.run_head(case, DEV)
    yard = to.head_yard(case)
    for k, r in to.check_head(case, got, yard).items():
        print(to.worst_ratio_line(f"head_bce {k} {to.head_id(case)}", r))
        _note(f"head_bce {k}", r, yard.get(k))
    to.check_head_chain(case, got, DEV)


@pytest.mark.parametrize("mode", ["exact", "float"])
@pytest.mark.parametrize("case", to.RR_CASES, ids=to.rr_id)
def test_reduce_rows(case, mode):
    r = to.check_rr(case, mode, to.run_rr(case, mode, DEV), bitwise=True)
    _note("reduce_rows", r)


@pytest.mark.parametrize("mode", ["exact", "float"])
@pytest.mark.parametrize("case", to.CS_CASES, ids=to.cs_id)
def test_colsum(case, mode):
    r = to.check_cs(case, mode, to.run_cs(case, mode, DEV))
    _note("colsum", r)


@pytest.mark.parametrize("case", to.DO_CASES, ids=to.do_id)
def test_dense_optimizer(case):
    yard = to.do_yard(case)
    r = to.check_do(case, to.run_do(case, DEV), yard, to.holder(DEV))
    print(to.worst_ratio_line(f"dense_optimizer {to.do_id(case)}", r))
    _note(f"dense_optimizer {case.opt}", r, yard)


@pytest.mark.parametrize("opt", to.DO_OPTS)
def test_dense_optimizer_found_inf_zero_equals_unflagged(opt):
    to.check_do_flag_zero(opt, DEV)


@pytest.mark.parametrize("mode", ["exact", "float"])
def test_dense_optimizer_slab_segments(mode):
    r = to.check_slab(mode, to.run_slab(mode, DEV))
    _note("dense_optimizer segments", r)


@pytest.mark.parametrize("case", to.CF_CASES, ids=to.cf_id)
def test_check_finite(case):
    to.check_cf(case, to.run_cf(case, DEV))


@pytest.mark.parametrize("n", to.CAST_NS)
def test_cast_bf16(n):
    to.check_cast(n, to.run_cast(n, DEV))


@pytest.mark.parametrize("case", to.AH_CASES, ids=to.ah_id)
def test_auc_hist(case):
    to.check_ah(case, to.run_ah(case, DEV))


def test_auc_hist_nb_limit_is_refused_and_device_stays_usable():
    """Host-side check: nothing is launched, the histogram stays as it was,
    and a valid call still passes. 8192 buckets (64 KiB of LDS) still run."""
    c = to.AHCase(200, 257)
    d = to.ah_data(c)
    x, y = d["x"].to(DEV), d["y"].to(DEV)
    for nb in (8193, 1 << 20, 0):
        h = torch.full((2 * nb,), 3, dtype=torch.int64, device=DEV)
        with pytest.raises(RuntimeError, match=r"1 <= nb <= 8192"):
            ops.auc_hist(x, y, nb, h)
        torch.cuda.synchronize()
        assert bool((h == 3).all())
    with pytest.raises(RuntimeError, match="must be a GPU tensor"):
        ops._native().auc_hist(x, d["y"], 200, torch.zeros(400, dtype=torch.int64, device=DEV))
    with pytest.raises(RuntimeError, match="fp32 contiguous"):
        ops.auc_hist(x, y.double(), 200, torch.zeros(400, dtype=torch.int64, device=DEV))
    h = torch.zeros(2 * 8192, dtype=torch.int64, device=DEV)
    ops.auc_hist(x, y, 8192, h)
    assert int(h.sum()) == c.n and int(h[8192:].sum()) == d["npos"]
    to.check_ah(c, to.run_ah(c, DEV))


@pytest.mark.parametrize("mode", ["exact", "float"])
@pytest.mark.parametrize("case", to.RA_CASES, ids=to.ra_id)
def test_reduce_adam(case, mode):
    got = to.run_ra(case, mode, DEV)
    yard = to.ra_yard(case, mode)
    r = to.check_ra(case, mode, got, True, yard, to.holder(DEV))
    _note("reduce_adam", r, yard)
    to.check_ra_same(case, mode, got, to.run_ra(case, mode, DEV, separate=True))


@pytest.mark.parametrize("F,D,B", to.GLUE_CASES)
def test_concat_features(F, D, B):
    to.check_concat(F, D, B, to.run_concat(F, D, B, DEV))


@pytest.mark.parametrize("pitched", [False, True])
@pytest.mark.parametrize("relu", [True, False])
@pytest.mark.parametrize("F,D,B", to.GLUE_CASES)
def test_split_features(F, D, B, relu, pitched):
    to.check_split(F, D, B, relu, to.run_split(F, D, B, relu, pitched, DEV))


@pytest.mark.parametrize("mode", ["exact", "float"])
@pytest.mark.parametrize("n,acc,add", to.CROSS_CASES)
def test_cross_bwd(n, acc, add, mode):
    r = to.check_cross(n, acc, add, mode, to.run_cross(n, acc, add, mode, DEV))
    _note("cross_bwd", r)


@pytest.mark.parametrize("B,nd,ni", to.BL_CASES)
def test_batch_load(B, nd, ni):
    to.check_bl(B, nd, ni, to.run_bl(B, nd, ni, DEV))
