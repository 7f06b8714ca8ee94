"""Cases and runners of the streaming attention kernels
(csrc/kernels/attention_stream.hip, 64 < T <= 4096), shared by
tests/test_gpu_attention_stream.py and its child tests/helpers/attn_stream_order.py.

The oracle is tests/encoder_oracle.py's (``eo``): float64 ``mha_fwd`` /
``mha_bwd`` / ``mha_lse`` and the bound of ``eo.assert_within``. At rate 0 a
case is ``eo.long_attn_case`` itself, which works at any T. With dropout and
T > 512 the case is built here from the rate-0 case's inputs and the mask of
row stride 4096 (``long_attn_case`` hard-codes 512, the stride below 513)."""
import functools
from types import SimpleNamespace

import torch

from tdfo_amd import ops
from tests import encoder_oracle as eo

DEV = "cuda"
NAN = float("nan")
SENTINEL = 12345.0
ORDER_ENV = "TDFO_ATTN_CAUSAL_ORDER"
STRIDE = 4096            # dropout row stride above T = 512

# (B, T, E, H, rate, pattern, causal, family, pad_id)
# one key in the ninth tile, nine whole tiles, one past them, 16 tiles, one past
EDGE_T = (513, 576, 577, 1024, 1025)
EDGE_CASES = [(2, T, 2 * dk, 2, 0.0, p, c, "randn", 0) for dk in eo.LONG_DK for T in EDGE_T
              for p in eo.PATTERNS for c in (False, True)]
HARD_CASES = [(2, T, 2 * dk, 2, 0.0, "left", c, f, 0) for f in eo.LONG_FAMILIES[1:]
              for T in (1087, 1024) for dk in (8, 64) for c in (False, True)]
# index and row-key range at the maximum (not arithmetic)
MAX_CASES = [(1, 4096, 16, 1, 0.0, "left", True, "randn", 0),
             (2, 4095, 8, 2, 0.0, "left", True, "randn", 0)]
DROP_SHAPES = [(2, 513, 16, 4), (1, 1025, 64, 1)]
DROP_CASES = [s + (r, "left", c, "randn", 0) for s in DROP_SHAPES for r in (0.1, 0.5)
              for c in (False, True)]
# causal grids B * H * nt (and twice that) that are no multiple of 8
TAIL_CASES = [s + (0.0, "left", True, "randn", 0) for s in [(3, 577, 12, 3), (1, 641, 32, 1)]]
PAD7_CASES = [(2, 577, 16, 2, 0.0, "left", c, "randn", 7) for c in (False, True)]
ORDER_CASES = TAIL_CASES + [(2, 1025, 16, 2, 0.0, "left", True, "randn", 0)]
# the shapes attention_long.hip also takes: the same bound, stride-512 mask
OVERLAP_CASES = [(2, T, 16, 2, r, "left", c, "randn", 0) for T in (65, 200, 512)
                 for r in (0.0, 0.1) for c in (False, True)]


@functools.lru_cache(maxsize=None)
def stream_case(B, T, E, H, rate, pattern, causal, family, pad_id=0):
    """CPU fp32 inputs and the fp64 oracle (out, dqkv, lse). Cached: read-only."""
    if rate == 0.0 or T <= ops.ATTN_LONG_MAXT:
        return eo.long_attn_case(B, T, E, H, rate, pattern, causal, family, pad_id)
    d = eo.long_attn_case(B, T, E, H, 0.0, pattern, causal, family, pad_id)
    m = eo.mul(eo.attn_keep(B, H, T, rate, eo.SEED, eo.STEP, stride=STRIDE), rate)
    exact = dict(out=eo.mha_fwd(d.qkv, d.valid, H, m, causal),
                 dqkv=eo.mha_bwd(d.qkv, d.valid, d.dout, H, m, causal), lse=d.exact["lse"])
    c = SimpleNamespace(**vars(d))
    c.rate, c.m, c.exact = rate, m, exact
    return c


def run_stream(c, step="case", rate=None):
    """attention_stream_fwd, then attention_stream_bwd on the forward's own out
    and lse, on device copies of case ``c`` -> {out, dqkv, lse} on the CPU. out,
    lse and the delta workspace are prefilled with NaN, dqkv with a sentinel."""
    qkv, ids, dout = (t.to(DEV).contiguous() for t in (c.qkv, c.ids, c.dout))
    out = torch.full((c.B, c.T, c.E), NAN, device=DEV)
    lse = torch.full((c.B, c.H, c.T), NAN, device=DEV)
    delta = torch.full((c.B, c.H, c.T), NAN, device=DEV)
    dqkv = torch.full((c.B, c.T, 3 * c.E), SENTINEL, device=DEV)
    step = c.step if step == "case" else step
    st = None if step is None else torch.tensor([step], dtype=torch.int64, device=DEV)
    rate = c.rate if rate is None else rate
    ops.attention_stream_fwd(qkv, ids, c.H, rate, c.seed, st, c.pad_id, out, lse, causal=c.causal)
    ops.attention_stream_bwd(qkv, ids, dout, c.H, rate, c.seed, st, c.pad_id, dqkv, out, lse,
                             delta, causal=c.causal)
    torch.cuda.synchronize()
    return dict(out=out.cpu(), dqkv=dqkv.cpu(), lse=lse.cpu())


def same(a, b):
    return all(torch.equal(a[k], b[k]) for k in ("out", "dqkv", "lse"))


def check_case(case):
    """every output written, within the oracle bound, dK of PAD keys exactly 0,
    and a second run bit-identical"""
    c = stream_case(*case)
    got = run_stream(c)
    assert not bool(torch.isnan(got["out"]).any()), "out not fully written"
    assert not bool(torch.isnan(got["lse"]).any()), "lse not fully written"
    assert not bool((got["dqkv"] == SENTINEL).any()), "dqkv not fully written"
    assert not bool(torch.isnan(got["dqkv"]).any()), "dqkv has NaN (delta not fully written?)"
    eo.assert_within(got, c, f"stream attention {case}")
    pad = (~c.valid)[:, :, None].expand(c.B, c.T, c.E)
    eo.check_exact_zero(got["dqkv"][..., c.E:2 * c.E], pad, "dK rows of PAD keys")
    assert same(got, run_stream(c)), "a second run differs"
    return c, got
