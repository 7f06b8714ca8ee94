"""CPU side of Bert4Rec beyond T = 64: the dropout hash's row keying, the
torch reference of the attention core at long T, and the CPU trainer the GPU
tests of tests/test_gpu_long_seq.py compare against."""
import math

import torch

from tdfo_amd import ops
from tdfo_amd.ops import reference as ref
from tests.test_bert4rec import _batch


def _keep_scale_stride(B, H, T, rate, seed, step, stride):
    """attn_keep_scale re-implemented with an explicit row stride."""
    a = (seed ^ ((step * 0x632BE5AB) & 0xFFFFFFFF)) & 0xFFFFFFFF
    bh = torch.arange(B * H, dtype=torch.int64).view(B, H, 1, 1)
    i = torch.arange(T, dtype=torch.int64).view(1, 1, T, 1)
    j = torch.arange(T, dtype=torch.int64).view(1, 1, 1, T)
    r = ref._hash3(torch.full((1,), a, dtype=torch.int64), bh * stride + i, j)
    keep = (r >> 8).to(torch.float32) * (1.0 / 16777216.0) >= rate
    return keep.to(torch.float32) / (1.0 - rate)


def test_long_rows_do_not_alias_the_next_head():
    """Keyed with stride 64, row (h = 0, i = 64) would get exactly the mask of
    row (h = 1, i = 0); above T = 64 the stride is 512."""
    m = ref.attn_keep_scale(1, 2, 100, 0.1, 123, 7, "cpu")
    assert not torch.equal(m[0, 0, 64], m[0, 1, 0])
    assert torch.equal(m, _keep_scale_stride(1, 2, 100, 0.1, 123, 7, 512))
    old = _keep_scale_stride(1, 2, 100, 0.1, 123, 7, 64)
    assert torch.equal(old[0, 0, 64], old[0, 1, 0])          # the defect this avoids


def test_short_rows_keep_stride_64():
    for B, H, T in [(2, 2, 20), (1, 4, 64), (3, 1, 7)]:
        got = ref.attn_keep_scale(B, H, T, 0.1, 123, 7, "cpu")
        assert torch.equal(got, _keep_scale_stride(B, H, T, 0.1, 123, 7, 64))


def _mha(qkv, ids, H):
    """The reference model's maths (as tests/test_gpu_attention.py::_mha_reference)."""
    B, T, E3 = qkv.shape
    E = E3 // 3
    dk = E // H
    q, k, v = qkv.view(B, T, 3, H, dk).permute(2, 0, 3, 1, 4)
    scores = q @ k.transpose(-2, -1) / math.sqrt(dk)
    mask = (ids != 0).view(B, 1, 1, T).repeat(1, 1, T, 1)
    scores = scores.masked_fill(mask == 0, -1e9)
    return (torch.softmax(scores, dim=-1) @ v).transpose(1, 2).reshape(B, T, E)


def test_cpu_attention_ops_at_long_T():
    torch.manual_seed(0)
    B, T, E, H = 2, 100, 16, 4
    qkv = torch.randn(B, T, 3 * E)
    ids = torch.randint(1, 50, (B, T))
    ids[:, : T // 3] = 0
    ids[0] = 0
    out = torch.empty(B, T, E)
    ops.attention_fwd(qkv, ids, H, 0.0, 1, None, 0, out, lse=None)
    x = qkv.clone().requires_grad_(True)
    exp = _mha(x, ids, H)
    assert torch.allclose(out, exp, atol=1e-5, rtol=1e-4)
    g = torch.randn_like(exp)
    exp.backward(g)
    dqkv = torch.empty_like(qkv)
    ops.attention_bwd(qkv, ids, g, H, 0.0, 1, None, 0, dqkv, out=out, lse=None)
    assert torch.allclose(dqkv, x.grad, atol=1e-4, rtol=1e-3)


def test_cpu_trainer_steps_at_the_paper_shape():
    from tdfo_amd.models.bert4rec import Bert4RecTrainer

    n, T, E, H, L, B = 300, 200, 64, 2, 1, 4
    tr = Bert4RecTrainer(n, T, E, H, L, B, lr=3e-3, device="cpu", seed=3)
    g = torch.Generator().manual_seed(0)
    for _ in range(3):
        s, l = _batch(g, B, T, n)
        tr.load_batch(s, l)
        tr.step()
    loss = tr.pop_loss()
    assert math.isfinite(loss) and loss > 0
