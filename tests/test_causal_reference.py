"""CPU reference of causal attention (ops.reference.attention_core(causal=True)):
the oracle the GPU kernels of tests/test_gpu_causal_attention.py are held to."""
import math

import pytest
import torch

from tdfo_amd import ops
from tdfo_amd.ops import reference as ref

SHAPES = [(2, 7, 32, 1), (2, 70, 16, 2)]


def _inputs(B, T, E, seed=0):
    g = torch.Generator().manual_seed(seed)
    qkv = torch.randn(B, T, 3 * E, generator=g)
    ids = torch.randint(0, 6, (B, T), generator=g)            # ~1/6 PAD, anywhere
    return qkv, ids


def _tril_attention(qkv, ids, H):
    """Explicit formulation: per query i a softmax over keys 0 .. i only, padded
    keys among them at -1e9."""
    B, T, E3 = qkv.shape
    E = E3 // 3
    dk = E // H
    q, k, v = qkv.view(B, T, 3, H, dk).permute(2, 0, 3, 1, 4)
    out = torch.zeros(B, H, T, dk)
    for i in range(T):
        s = (q[:, :, i:i + 1] / math.sqrt(dk)) @ k[:, :, :i + 1].transpose(-2, -1)   # [B,H,1,i+1]
        s = s.masked_fill((ids[:, :i + 1] == 0).view(B, 1, 1, i + 1), -1e9)
        out[:, :, i] = (torch.softmax(s, -1) @ v[:, :, :i + 1])[:, :, 0]
    return out.transpose(1, 2).reshape(B, T, E)


@pytest.mark.parametrize("B,T,E,H", SHAPES)
def test_causal_core_equals_explicit_tril(B, T, E, H):
    qkv, ids = _inputs(B, T, E)
    got = ref.attention_core(qkv, ids, H, 0.0, 1, 0, 0, causal=True)
    torch.testing.assert_close(got, _tril_attention(qkv, ids, H), rtol=1e-5, atol=1e-6)
    # the ops-level CPU path passes the flag through, forward and backward
    out = torch.empty(B, T, E)
    ops.attention_fwd(qkv, ids, H, 0.0, 1, None, 0, out, causal=True)
    assert torch.equal(out, got)
    x = qkv.clone().requires_grad_(True)
    g = torch.randn(B, T, E, generator=torch.Generator().manual_seed(1))
    _tril_attention(x, ids, H).backward(g)
    d = torch.empty_like(qkv)
    ops.attention_bwd(qkv, ids, g, H, 0.0, 1, None, 0, d, causal=True)
    torch.testing.assert_close(d, x.grad, rtol=1e-4, atol=1e-5)


@pytest.mark.parametrize("B,T,E,H", SHAPES)
def test_causal_false_is_the_old_call(B, T, E, H):
    qkv, ids = _inputs(B, T, E)
    for rate in (0.0, 0.1):
        a = ref.attention_core(qkv, ids, H, rate, 5, 3, 0)
        b = ref.attention_core(qkv, ids, H, rate, 5, 3, 0, causal=False)
        assert torch.equal(a, b)
    c = ref.attention_core(qkv, ids, H, 0.0, 5, 3, 0, causal=True)
    assert not torch.equal(a, c)


@pytest.mark.parametrize("B,T,E,H", SHAPES)
def test_left_padded_prefix_rows_are_uniform_over_visible_keys(B, T, E, H):
    """Rows i < p of a sequence left-padded by p see PAD keys only: uniform
    1 / (i + 1) over keys 0 .. i, not 1 / T. Read off with one-hot V: dim d of a
    head marks key d, so out[b, i, h, d] = P[b, h, i, d]."""
    qkv, ids = _inputs(B, T, E)
    dk = E // H
    p = min(dk, T // 2)
    ids = ids.clamp(min=1)
    ids[:, :p] = 0
    x = qkv.clone().view(B, T, 3, H, dk)
    x[:, :, 2] = 0.0
    n = min(dk, T)
    x[:, torch.arange(n), 2, :, torch.arange(n)] = 1.0
    out = ref.attention_core(x.view(B, T, 3 * E), ids, H, 0.0, 1, 0, 0, causal=True)
    P = out.view(B, T, H, dk)                                  # [b, i, h, key d]
    for i in range(p):
        exp = torch.zeros(dk)
        exp[: i + 1] = 1.0 / (i + 1)
        torch.testing.assert_close(P[:, i], exp.expand(B, H, dk), rtol=1e-6, atol=1e-7)
    # the first valid row sees exactly itself among PADs: all weight on key p
    if p < n:
        assert torch.allclose(P[:, p, :, p], torch.ones(B, H))


@pytest.mark.parametrize("B,T,E,H", SHAPES)
def test_no_leak_from_later_positions(B, T, E, H):
    qkv, ids = _inputs(B, T, E)
    for rate in (0.0, 0.1):
        base = ref.attention_core(qkv, ids, H, rate, 9, 2, 0, causal=True)
        for i0 in (0, T // 2, T - 2):
            other = qkv.clone()
            other[:, i0 + 1:] = torch.randn(B, T - i0 - 1, 3 * E,
                                            generator=torch.Generator().manual_seed(i0 + 7))
            got = ref.attention_core(other, ids, H, rate, 9, 2, 0, causal=True)
            assert torch.equal(got[:, : i0 + 1], base[:, : i0 + 1])
            assert not torch.equal(got[:, i0 + 1:], base[:, i0 + 1:])
