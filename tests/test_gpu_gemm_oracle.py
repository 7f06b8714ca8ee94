"""The bf16 GEMM kernels (csrc/kernels/gemm.hip) against the float64 oracles
of tests/dense_oracle.py: every case through the HIP kernels under every GEMM
policy (0 auto, 1 two-stage 64/128-row, 2 deep ring, 3 ping-pong, 4 256x128,
5 DCN-v2 routing, 8 two-group 256x128). Pairs run under the policies for
which a paired launch forms (dense_oracle.PAIR_RUNS). Exact mode everywhere -- integer data
whose every partial sum is representable, so results must equal the oracle
and bf16 outputs its round-to-nearest-even, with no tolerance -- and float
mode (randn, derived per-element bounds) on the K sweep, the split cases and
three epilogues. Operands sit in NaN-filled parents and outputs in
sentinel-filled ones: a clamped or stray read that reaches a result, a write
outside [M, N] and an element never written all fail."""
import pytest
import torch

from tdfo_amd import ops
from tests import dense_oracle as do

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
POLICIES = (0, 1, 2, 3, 4, 5, 8)
WORST = {}                       # policy -> worst float-mode error / bound


@pytest.fixture(params=POLICIES, ids=lambda p: f"pol{p}")
def policy(request):
    old = ops.gemm_policy(request.param)
    yield request.param
    ops.gemm_policy(old)


def _note(policy, ratio):
    WORST[policy] = max(WORST.get(policy, 0.0), ratio)


@pytest.fixture(scope="module", autouse=True)
def report_worst_ratios():
    """After the file's tests: the worst float-mode error / bound per policy
    (shown with -s)."""
    yield
    for p in sorted(WORST):
        print(do.worst_ratio_line(f"policy {p}", WORST[p]))


@pytest.mark.parametrize("case", do.ALL_CASES, ids=do.case_id)
def test_gemm_exact(case, policy):
    got = do.run_gemm(case, DEV, mode="exact")
    do.check_gemm(got, do.gemm_oracle(case, "exact"), "exact")


@pytest.mark.parametrize("case", do.FLOAT_CASES, ids=do.case_id)
def test_gemm_float_within_bound(case, policy):
    got = do.run_gemm(case, DEV, mode="float")
    ratio = do.check_gemm(got, do.gemm_oracle(case, "float"), "float")
    print(do.worst_ratio_line(f"pol{policy} {do.case_id(case)}", ratio))
    _note(policy, ratio)
    assert ratio <= 1.0


PAIR_PARAMS = [(n, p, m) for n, p in do.PAIR_RUNS for m in do.PAIR_MODES[n]]


@pytest.mark.parametrize("pairing", [1, 0])
@pytest.mark.parametrize("pair,pol,mode", PAIR_PARAMS,
                         ids=[f"{n}-pol{p}-{m}" for n, p, m in PAIR_PARAMS])
def test_gemm_batch_pairs(pair, pol, mode, pairing):
    """Paired launches against the oracle (not merely against two launches),
    under the policies for which the pair forms (dense_oracle.PAIR_RUNS):
    the ping-pong, 256x128 and two-group pair kernels, unequal grids,
    split-K slabs (one empty) and column sums beside a zero-heavy mask."""
    cases = do.PAIRS[pair]
    for c, got in zip(cases, do.run_pair(cases, DEV, policy=pol, mode=mode, pairing=pairing)):
        ratio = do.check_gemm(got, do.gemm_oracle(c, mode), mode)
        _note(pol, ratio)
        assert ratio <= 1.0


@pytest.mark.parametrize("mode", ["exact", "float"])
def test_linear_wrappers(mode, policy):
    ratio = do.check_wrappers(DEV, mode)
    _note(policy, ratio)
    assert ratio <= 1.0


def test_split_with_epilogue_is_refused_and_device_stays_usable():
    """Host-side check: nothing is launched, and a valid call still passes."""
    c = do.SPLIT_CASES[2]
    ins, outp = do.stage(c, "exact", DEV)
    o = do.case_data(c, "exact")["out"]["c32"].view(outp["c32"])
    before = outp["c32"].clone()
    bias = torch.ones(c.N, device=DEV)
    mask = torch.ones(c.M, c.N, dtype=torch.bfloat16, device=DEV)
    for kw in (dict(bias=bias), dict(relu=True), dict(mask=mask)):
        with pytest.raises(RuntimeError, match="splits > 1 takes no bias, relu or mask"):
            ops.gemm(ins["a"], c.a_col, ins["b"], c.b_col, out32=o, splits=c.S, ldc32=c.ld32, **kw)
    torch.cuda.synchronize()
    assert torch.equal(outp["c32"].view(torch.int32), before.view(torch.int32))
    do.check_gemm(do.run_gemm(c, DEV), do.gemm_oracle(c, "exact"), "exact")
