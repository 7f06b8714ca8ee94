"""Causal attention on MI355X: the one-wave kernel (T <= 64, attention.hip) and
the tiled kernels (64 < T <= 512, attention_long.hip) with AttnArgs::causal,
against ops.reference.attention_core(causal=True). Tolerances are those of the
non-causal attention tests against the same kind of oracle (forward 1e-5 /
1e-4, backward 1e-4 / 1e-3)."""
import pytest
import torch

from tdfo_amd import ops
from tdfo_amd.ops import reference as ref

pytestmark = pytest.mark.gpu
DEV = "cuda"

SHORT = [(16, 20, 16, 2), (3, 64, 64, 4), (5, 7, 32, 1)]
# (2, 65, 16, 2): one row past a tile edge; (2, 100, 16, 4): d_k = 4; (3, 128, 64, 4): whole
# tiles; (2, 200, 64, 2): partial last tile; (1, 512, 64, 1): maximum T, d_k = 64
LONG = [(2, 65, 16, 2), (2, 100, 16, 4), (3, 128, 64, 4), (2, 200, 64, 2), (1, 512, 64, 1)]
PATTERNS = ("left", "full", "lone", "right")


@pytest.fixture(scope="module", autouse=True)
def _native():
    from tdfo_amd.ops import _ext

    assert _ext.load(), "native library must load on the GPU box"


def _attn(qkv, ids, H, rate=0.0, seed=1, step=None, causal=True):
    B, T, E3 = qkv.shape
    out = torch.empty(B, T, E3 // 3, device=DEV)
    lse = torch.empty(B, H, T, device=DEV)
    ops.attention_fwd(qkv, ids, H, rate, seed, step, 0, out, lse=lse, causal=causal)
    return out, lse


def _attn_bwd(qkv, ids, g, H, out, lse, rate=0.0, seed=1, step=None, causal=True):
    d = torch.empty_like(qkv)
    ops.attention_bwd(qkv, ids, g, H, rate, seed, step, 0, d, out=out, lse=lse, causal=causal)
    return d


def _ids(B, T, pattern):
    """left: the first T // 3 ids of every sequence are PAD (uniform prefix
    rows); full: as left, and every id of sequence 0 is PAD; lone: as left, and
    sequence 0's only valid key is the last; right: the last T // 3 ids are PAD."""
    ids = torch.randint(1, 50, (B, T), device=DEV)
    if pattern == "right":
        ids[:, T - T // 3:] = 0
        return ids
    ids[:, : T // 3] = 0
    if pattern == "full":
        ids[0] = 0
    elif pattern == "lone":
        ids[0] = 0
        ids[0, T - 1] = 7
    return ids


def _reference(qkv, ids, H, g, rate=0.0, seed=1, step=0):
    x = qkv.clone().requires_grad_(True)
    exp = ref.attention_core(x, ids, H, rate, seed, step, 0, causal=True)
    exp.backward(g)
    return exp.detach(), x.grad


@pytest.mark.parametrize("B,T,E,H", SHORT + LONG)
def test_causal_attention_matches_reference(B, T, E, H):
    torch.manual_seed(0)
    for pattern in PATTERNS:
        qkv = torch.randn(B, T, 3 * E, device=DEV)
        ids = _ids(B, T, pattern)
        g = torch.randn(B, T, E, device=DEV)
        exp, dexp = _reference(qkv, ids, H, g)
        out, lse = _attn(qkv, ids, H)
        print(pattern, "fwd max err", float((out - exp).abs().max()))
        assert torch.allclose(out, exp, atol=1e-5, rtol=1e-4), pattern
        dqkv = _attn_bwd(qkv, ids, g, H, out, lse)
        print(pattern, "bwd max err", float((dqkv - dexp).abs().max()))
        assert torch.allclose(dqkv, dexp, atol=1e-4, rtol=1e-3), pattern
    # and the flag does something: the full softmax differs
    full, _ = _attn(qkv, ids, H, causal=False)
    assert not torch.allclose(full, out, atol=1e-3)


@pytest.mark.parametrize("B,T,E,H", [(2, 20, 16, 2), (2, 200, 64, 2)])
def test_causal_attention_exact_no_leak(B, T, E, H):
    """Bit-exact: later rows of q, k, v cannot reach earlier outputs, and
    queries with no upstream gradient give later keys exactly none. Finite
    values (0 * NaN in the diagonal tile's P~.V would say nothing)."""
    torch.manual_seed(3)
    qkv = torch.randn(B, T, 3 * E, device=DEV)
    ids = _ids(B, T, "left")
    out, lse = _attn(qkv, ids, H)
    for i0 in (0, 63, 64, 130):
        if i0 >= T:
            continue
        other = qkv.clone()
        other[:, i0 + 1:] = torch.randn(B, T - i0 - 1, 3 * E, device=DEV) * 3
        out2, lse2 = _attn(other, ids, H)
        assert torch.equal(out2[:, : i0 + 1], out[:, : i0 + 1]), i0
        if T > ops.ATTN_SHORT_MAXT:                    # (the one-wave kernel writes no lse)
            assert torch.equal(lse2[..., : i0 + 1], lse[..., : i0 + 1]), i0
        if i0 + 1 < T:
            assert not torch.equal(out2[:, i0 + 1:], out[:, i0 + 1:])
        g = torch.randn(B, T, E, device=DEV)
        g[:, i0:] = 0.0
        d = _attn_bwd(qkv, ids, g, H, out, lse)
        kv = d[:, i0:, E:]
        assert bool((kv == 0).all()), (i0, float(kv.abs().max()))
        if i0 > 0:
            assert bool((d[:, :i0, E:] != 0).any())


@pytest.mark.parametrize("B,T,E,H", [(2, 130, 32, 2), (4, 20, 16, 2)])
def test_causal_attention_dropout_matches_hash_reference(B, T, E, H):
    torch.manual_seed(1)
    rate = 0.1
    qkv = torch.randn(B, T, 3 * E, device=DEV)
    ids = torch.randint(0, 30, (B, T), device=DEV)
    step = torch.tensor([7], dtype=torch.int64, device=DEV)
    g = torch.randn(B, T, E, device=DEV)
    exp, dexp = _reference(qkv, ids, H, g, rate, 123, 7)
    out, lse = _attn(qkv, ids, H, rate, 123, step)
    assert torch.allclose(out, exp, atol=1e-5, rtol=1e-4)
    d = _attn_bwd(qkv, ids, g, H, out, lse, rate, 123, step)
    assert torch.allclose(d, dexp, atol=1e-4, rtol=1e-3)
    # The mask is the non-causal one restricted to j <= i, read off the kernel
    # itself: with no padding and V one-hot (dim d of a head marks key s d)
    # out[b, i, h, d] = P~[b, h, i, s d], which is 0 exactly where the mask
    # dropped it or the key lies in the future.
    dk = E // H
    keys = torch.arange(dk, device=DEV) * (T // dk)
    ids1 = torch.ones(B, T, dtype=torch.int64, device=DEV)
    q1 = qkv.clone().view(B, T, 3, H, dk)
    q1[:, :, 2] = 0.0
    q1[:, keys, 2, :, torch.arange(dk, device=DEV)] = 1.0
    q1 = q1.view(B, T, 3 * E)
    o1, _ = _attn(q1, ids1, H, rate, 123, step)
    zero = o1.view(B, T, H, dk) == 0                                       # [b, i, h, d]
    keep = ref.attn_keep_scale(B, H, T, rate, 123, 7, DEV)[:, :, :, keys]    # [b, h, i, d]
    future = keys[None, :] > torch.arange(T, device=DEV)[:, None]          # [i, d]
    exp_zero = (keep.permute(0, 2, 1, 3) == 0) | future[None, :, None, :]
    assert torch.equal(zero, exp_zero)
    seen = ~future[None, :, None, :].expand_as(zero)
    assert 0.0 < float(zero[seen].float().mean()) < 2 * rate


def test_causal_attention_is_deterministic():
    torch.manual_seed(2)
    B, T, E, H = 3, 200, 64, 2
    qkv = torch.randn(B, T, 3 * E, device=DEV)
    ids = _ids(B, T, "full")
    step = torch.tensor([3], dtype=torch.int64, device=DEV)
    out, lse = _attn(qkv, ids, H, 0.1, 5, step)
    out_b, lse_b = _attn(qkv, ids, H, 0.1, 5, step)
    assert torch.equal(out, out_b) and torch.equal(lse, lse_b)
    g = torch.randn_like(out)
    a = _attn_bwd(qkv, ids, g, H, out, lse, 0.1, 5, step)
    b = _attn_bwd(qkv, ids, g, H, out, lse, 0.1, 5, step)
    assert torch.equal(a, b)


def test_causal_attention_argument_errors_leave_device_usable():
    """Host-side checks: nothing is launched, and a valid call still passes."""
    E, H = 16, 2
    qkv = torch.randn(2, 100, 3 * E, device=DEV)
    ids = torch.ones(2, 100, dtype=torch.int64, device=DEV)
    out = torch.empty(2, 100, E, device=DEV)
    with pytest.raises(ValueError, match="lse"):
        ops.attention_fwd(qkv, ids, H, 0.0, 1, None, 0, out, causal=True)
    with pytest.raises(ValueError, match="lse"):
        ops.attention_bwd(qkv, ids, out, H, 0.0, 1, None, 0, torch.empty_like(qkv), causal=True)
    got, _ = _attn(qkv, ids, H)
    exp = ref.attention_core(qkv, ids, H, 0.0, 1, 0, 0, causal=True)
    assert torch.allclose(got, exp, atol=1e-5, rtol=1e-4)
