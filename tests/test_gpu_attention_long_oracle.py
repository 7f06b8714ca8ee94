"""The tiled attention kernels (csrc/kernels/attention_long.hip, 64 < T <= 512)
on MI355X against the float64 oracles of tests/encoder_oracle.py: ``out``,
``dqkv`` and the saved ``lse`` at every d_k (operand widths scalar / float2 /
float4, 1 / 2 / 4 column blocks) and every tile geometry (one key past a tile,
whole tiles, T = 511 and 512), non-causal and causal, four id patterns, inputs
whose scores reach +-20 .. 80 with the row maximum arriving in the last tile or
sitting in the first, dropout 0.1 and 0.5, causal grids that are no multiple
of 8 (the tail of al_causal_block), pad_id = 7, and the natural block order.

Bound, ``out`` and ``dqkv``: row_err(kernel) <= max(8 * row_err(fp32
reference), 2^-20). ``lse``: the same bound on max |got - exact| / max(1,
|exact|) over the rows that see a valid key, the reference being the fp32
log-sum-exp of the reference's own scores; a row whose visible keys are all
PAD must lie under the backward's -5e8 threshold and within 32 (half an f32
ulp at 1e9) of the exact -1e9 + log n. Every test prints kernel error,
reference error and their ratio per tensor; profiles/attention_long_oracle.md
records the worst ratios of one run."""
import os
import subprocess
import sys

import pytest
import torch

from tdfo_amd import ops
from tests import encoder_oracle as eo

pytestmark = pytest.mark.gpu
DEV = "cuda"
NAN = float("nan")
SENTINEL = 12345.0
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ORDER_ENV = "TDFO_ATTN_CAUSAL_ORDER"


@pytest.fixture(scope="module", autouse=True)
def _native():
    from tdfo_amd.ops import _ext

    assert _ext.load(), "native library must load on the GPU box"


def run_long(c, step="case", rate=None):
    """attention_fwd, then attention_bwd on the forward's own out and lse, on
    device copies of case ``c`` -> {out, dqkv, lse} on the CPU. out and lse
    are prefilled with NaN, dqkv with a sentinel."""
    qkv, ids, dout = (t.to(DEV).contiguous() for t in (c.qkv, c.ids, c.dout))
    out = torch.full((c.B, c.T, c.E), NAN, device=DEV)
    lse = torch.full((c.B, c.H, c.T), NAN, device=DEV)
    dqkv = torch.full((c.B, c.T, 3 * c.E), SENTINEL, device=DEV)
    step = c.step if step == "case" else step
    st = None if step is None else torch.tensor([step], dtype=torch.int64, device=DEV)
    rate = c.rate if rate is None else rate
    ops.attention_fwd(qkv, ids, c.H, rate, c.seed, st, c.pad_id, out, lse=lse, causal=c.causal)
    ops.attention_bwd(qkv, ids, dout, c.H, rate, c.seed, st, c.pad_id, dqkv, out=out, lse=lse,
                      causal=c.causal)
    torch.cuda.synchronize()
    return dict(out=out.cpu(), dqkv=dqkv.cpu(), lse=lse.cpu())


def _same(a, b):
    return all(torch.equal(a[k], b[k]) for k in ("out", "dqkv", "lse"))


@pytest.mark.parametrize("case", eo.LONG_CASES, ids=str)
def test_long_attention_matches_oracle(case):
    c = eo.long_attn_case(*case)
    assert c.T > ops.ATTN_SHORT_MAXT
    got = run_long(c)
    assert not bool(torch.isnan(got["out"]).any()), "out not fully written"
    assert not bool(torch.isnan(got["lse"]).any()), "lse not fully written"
    assert not bool((got["dqkv"] == SENTINEL).any()), "dqkv not fully written"
    eo.assert_within(got, c, f"long attention {case}")
    E = c.E
    pad = (~c.valid)[:, :, None].expand(c.B, c.T, E)
    eo.check_exact_zero(got["dqkv"][..., E:2 * E], pad, "dK rows of PAD keys")
    assert _same(got, run_long(c)), "a second run differs"


@pytest.mark.parametrize("causal", [False, True])
@pytest.mark.parametrize("shape", [(2, 129, 16, 4), (2, 200, 64, 2)])
def test_long_attention_step_and_rate(shape, causal):
    """step=None is step 0; another step draws another mask, which moves out
    and dqkv but not lse (l is accumulated without the mask), and so does the
    rate: lse is the one output that must not depend on dropout"""
    c = eo.long_attn_case(*shape, 0.1, "left", causal, "randn")
    none, zero, case = run_long(c, step=None), run_long(c, step=0), run_long(c)
    assert _same(none, zero)
    assert not torch.equal(zero["out"], case["out"]) and not torch.equal(zero["dqkv"], case["dqkv"])
    assert torch.equal(zero["lse"], case["lse"])
    # step 0 against the oracle with the step-0 mask
    m0 = eo.mul(eo.attn_keep(c.B, c.H, c.T, c.rate, c.seed, 0, stride=512), c.rate)
    ref = eo.ref_err(c)
    assert eo.row_err(zero["out"], eo.mha_fwd(c.qkv, c.valid, c.H, m0, causal)) <= eo.bound(ref["out"])
    assert eo.row_err(zero["dqkv"], eo.mha_bwd(c.qkv, c.valid, c.dout, c.H, m0, causal)) \
        <= eo.bound(ref["dqkv"])
    for rate in (0.0, 0.5):
        other = run_long(c, rate=rate)
        assert torch.equal(other["lse"], case["lse"]), rate
        assert not torch.equal(other["out"], case["out"]), rate
    dry = eo.long_attn_case(*shape, 0.0, "left", causal, "randn")
    assert torch.equal(dry.qkv, c.qkv)
    eo.assert_within(run_long(c, rate=0.0), dry, f"long attention {shape} rate 0 of the 0.1 case")


def test_long_attention_natural_block_order_is_bit_identical(tmp_path):
    """TDFO_ATTN_CAUSAL_ORDER=natural (read once per process: a child) gives
    the results of the default longest-first order, bit for bit, on the causal
    grids with a tail and on the paper shape"""
    assert os.environ.get(ORDER_ENV) != "natural", "the parent must run the default order"
    path = tmp_path / "natural.pt"
    env = dict(os.environ)
    env[ORDER_ENV] = "natural"
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "helpers", "attn_long_order.py"),
                        str(path)], cwd=ROOT, env=env, capture_output=True, text=True, timeout=170)
    assert r.returncode == 0, (r.returncode, r.stdout[-1000:], r.stderr[-2000:])
    natural = torch.load(path)
    assert len(natural) == len(eo.LONG_ORDER_CASES) == 6
    for case, nat in zip(eo.LONG_ORDER_CASES, natural):
        c = eo.long_attn_case(*case)
        assert c.causal
        got = run_long(c)
        for k in ("out", "lse", "dqkv"):
            assert torch.equal(got[k], nat[k]), (case, k)
