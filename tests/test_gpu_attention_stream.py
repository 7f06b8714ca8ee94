"""The streaming attention kernels (csrc/kernels/attention_stream.hip,
64 < T <= 4096) on MI355X against the float64 oracles of
tests/encoder_oracle.py: ``out``, ``dqkv`` and the saved ``lse`` at every d_k
and at T around the ninth and the seventeenth 64-key tile, non-causal and
causal, four id patterns, the hard input families at 17 tiles, the maximum T
(index and row-key range), dropout 0.1 and 0.5 against the stride-4096 mask,
causal grids with a tail, pad_id = 7, the natural block order, the shapes the
older tiled family also takes, and the argument errors.

Bound (eo.assert_within): row_err(kernel) <= max(8 * row_err(fp32 reference),
2^-20) for ``out`` and ``dqkv``; the same on ``lse`` over the rows that see a
valid key, and a row whose visible keys are all PAD under the backward's -5e8
threshold and within 32 of the exact -1e9 + log n. Every test prints kernel
error, reference error and their ratio per tensor."""
import os
import subprocess
import sys

import pytest
import torch

from tdfo_amd import ops
from tests import attention_stream_cases as sc
from tests import encoder_oracle as eo

pytestmark = pytest.mark.gpu
DEV = sc.DEV
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module", autouse=True)
def _native():
    from tdfo_amd.ops import _ext

    assert _ext.load(), "native library must load on the GPU box"


@pytest.mark.parametrize("case", sc.EDGE_CASES, ids=str)
def test_stream_attention_edges(case):
    c, _ = sc.check_case(case)
    assert c.T > ops.ATTN_LONG_MAXT


@pytest.mark.parametrize("case", sc.HARD_CASES, ids=str)
def test_stream_attention_hard_families(case):
    """`peaked` rows are nearly one-hot (P = 0.995 on one key): dS = P (dP - D)
    subtracts two MFMA chains of about 10 that differ by 0.05. With D = dO . O
    alone (2, 1087, 128, 2) causal missed the bound on ``dqkv`` (1.129e-4
    against the reference's 1.067e-5, ratio 10.58); the dQ role's correction by
    the row sum of dS brings it to 8.2e-6 (profiles/attention_stream.md)."""
    c, _ = sc.check_case(case)
    lo, hi = eo.LONG_SCORE_RANGE
    assert lo <= c.smax <= hi


@pytest.mark.parametrize("case", sc.MAX_CASES, ids=str)
def test_stream_attention_at_the_maximum(case):
    sc.check_case(case)


@pytest.mark.parametrize("case", sc.TAIL_CASES + sc.PAD7_CASES, ids=str)
def test_stream_attention_grid_tails_and_pad_id(case):
    sc.check_case(case)


@pytest.mark.parametrize("case", sc.DROP_CASES, ids=str)
def test_stream_attention_dropout(case):
    """against the oracle with the mask of row stride 4096; lse must not depend
    on rate or step, step=None is step 0, and the rate-0 run of the same inputs
    meets the rate-0 oracle"""
    c, got = sc.check_case(case)
    B, T, E, H, rate, pattern, causal, family, pad = case
    assert T > ops.ATTN_LONG_MAXT and torch.equal(c.m != 0, eo.attn_keep(B, H, T, rate, c.seed,
                                                                        c.step, stride=4096))
    none, zero = sc.run_stream(c, step=None), sc.run_stream(c, step=0)
    assert sc.same(none, zero)
    assert not torch.equal(zero["out"], got["out"]) and not torch.equal(zero["dqkv"], got["dqkv"])
    assert torch.equal(zero["lse"], got["lse"])
    m0 = eo.mul(eo.attn_keep(B, H, T, rate, c.seed, 0, stride=4096), rate)
    ref = eo.ref_err(c)
    assert eo.row_err(zero["out"], eo.mha_fwd(c.qkv, c.valid, H, m0, causal)) <= eo.bound(ref["out"])
    assert eo.row_err(zero["dqkv"], eo.mha_bwd(c.qkv, c.valid, c.dout, H, m0, causal)) \
        <= eo.bound(ref["dqkv"])
    dry = sc.stream_case(B, T, E, H, 0.0, pattern, causal, family, pad)
    assert torch.equal(dry.qkv, c.qkv)
    other = sc.run_stream(c, rate=0.0)
    assert torch.equal(other["lse"], got["lse"]) and not torch.equal(other["out"], got["out"])
    eo.assert_within(other, dry, f"stream attention {case} at rate 0")


@pytest.mark.parametrize("case", sc.OVERLAP_CASES, ids=str)
def test_stream_attention_on_the_tiled_family_shapes(case):
    """64 < T <= 512: the same bound; with dropout, eo.long_attn_case's own
    stride-512 oracle (the mask ops.attention_fwd draws at that shape)"""
    c, _ = sc.check_case(case)
    assert ops.ATTN_SHORT_MAXT < c.T <= ops.ATTN_LONG_MAXT


def test_stream_attention_natural_block_order_is_bit_identical(tmp_path):
    """TDFO_ATTN_CAUSAL_ORDER=natural (read once per process: a child) gives
    the results of the default longest-first order, bit for bit"""
    assert os.environ.get(sc.ORDER_ENV) != "natural", "the parent must run the default order"
    path = tmp_path / "natural.pt"
    env = dict(os.environ)
    env[sc.ORDER_ENV] = "natural"
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "helpers", "attn_stream_order.py"),
                        str(path)], cwd=ROOT, env=env, capture_output=True, text=True, timeout=170)
    assert r.returncode == 0, (r.returncode, r.stdout[-1000:], r.stderr[-2000:])
    natural = torch.load(path)
    assert len(natural) == len(sc.ORDER_CASES) == 3
    for case, nat in zip(sc.ORDER_CASES, natural):
        c = sc.stream_case(*case)
        assert c.causal
        got = sc.run_stream(c)
        for k in ("out", "lse", "dqkv"):
            assert torch.equal(got[k], nat[k]), (case, k)


def test_stream_attention_argument_errors_leave_device_usable():
    """T = 64, T = 4097, a missing delta and d_k = 2 raise ValueError and launch
    nothing (the prefilled outputs stay untouched); a valid call then passes"""
    H, E = 2, 16

    def bufs(T, H=H):
        qkv = torch.randn(1, T, 3 * E, device=DEV)
        ids = torch.ones(1, T, dtype=torch.int64, device=DEV)
        out = torch.full((1, T, E), sc.SENTINEL, device=DEV)
        lse = torch.full((1, H, T), sc.SENTINEL, device=DEV)
        return qkv, ids, out, lse

    for T in (64, 4097):
        qkv, ids, out, lse = bufs(T)
        with pytest.raises(ValueError, match="4096"):
            ops.attention_stream_fwd(qkv, ids, H, 0.0, 1, None, 0, out, lse)
        with pytest.raises(ValueError, match="4096"):
            ops.attention_stream_bwd(qkv, ids, out, H, 0.0, 1, None, 0, torch.empty_like(qkv), out,
                                     lse, torch.empty_like(lse))
        torch.cuda.synchronize()
        assert bool((out == sc.SENTINEL).all()) and bool((lse == sc.SENTINEL).all())
    qkv, ids, out, lse = bufs(577)
    dqkv = torch.full_like(qkv, sc.SENTINEL)
    with pytest.raises(ValueError, match="delta"):
        ops.attention_stream_bwd(qkv, ids, out, H, 0.0, 1, None, 0, dqkv, out, lse, None)
    with pytest.raises(ValueError, match="delta"):
        ops.attention_stream_bwd(qkv, ids, out, H, 0.0, 1, None, 0, dqkv, out, lse,
                                 torch.empty(1, H, 576, device=DEV))
    with pytest.raises(ValueError, match="lse"):
        ops.attention_stream_fwd(qkv, ids, H, 0.0, 1, None, 0, out, None)
    qkv8, ids8, out8, lse8 = bufs(577, H=8)                    # d_k = 2
    with pytest.raises(ValueError, match="d_k"):
        ops.attention_stream_fwd(qkv8, ids8, 8, 0.0, 1, None, 0, out8, lse8)
    torch.cuda.synchronize()
    assert bool((dqkv == sc.SENTINEL).all()) and bool((out == sc.SENTINEL).all())
    assert bool((out8 == sc.SENTINEL).all())
    sc.check_case(sc.PAD7_CASES[1])
