"""Bert4Rec beyond T = 64 on MI355X: the tiled attention core
(csrc/kernels/attention_long.hip), the wide-row LayerNorm / sequence prologue
(layernorm.hip, 1024 < n <= 32768) and the model / trainer on top of them.
Before these kernels every test here stopped at `attention: T > 64` or
`layernorm: n > 1024`."""
import pytest
import torch

from tdfo_amd import ops
from tdfo_amd.ops import reference as ref
from tests.test_bert4rec import _batch
from tests.test_gpu_attention import _mha_reference

pytestmark = pytest.mark.gpu
DEV = "cuda"


@pytest.fixture(scope="module", autouse=True)
def _native():
    from tdfo_amd.ops import _ext

    assert _ext.load(), "native library must load on the GPU box"


def _attn(qkv, ids, H, rate=0.0, seed=1, step=None):
    B, T, E3 = qkv.shape
    out = torch.empty(B, T, E3 // 3, device=DEV)
    lse = torch.empty(B, H, T, device=DEV)
    ops.attention_fwd(qkv, ids, H, rate, seed, step, 0, out, lse=lse)
    return out, lse


def _attn_bwd(qkv, ids, g, H, out, lse, rate=0.0, seed=1, step=None):
    d = torch.empty_like(qkv)
    ops.attention_bwd(qkv, ids, g, H, rate, seed, step, 0, d, out=out, lse=lse)
    return d


def _ids(B, T, pattern):
    """Every sequence left-padded by T // 3; sequence 0 then follows `pattern`:
    "left" (as the others), "full" (fully padded: a uniform softmax over all T
    keys) or "lone" (its only valid key is the last one, in the last tile)."""
    ids = torch.randint(1, 50, (B, T), device=DEV)
    ids[:, : T // 3] = 0
    if pattern == "full":
        ids[0] = 0
    elif pattern == "lone":
        ids[0] = 0
        ids[0, T - 1] = 7
    return ids


# (2, 65, 16, 2): one key and one query past the tile edge; (2, 100, 16, 4): d_k = 4;
# (3, 128, 64, 4): whole tiles, d_k = 16; (2, 200, 64, 2): the paper shape, d_k = 32, partial
# last tile; (1, 512, 64, 1): maximum T, d_k = 64
@pytest.mark.parametrize("B,T,E,H", [(2, 65, 16, 2), (2, 100, 16, 4), (3, 128, 64, 4),
                                     (2, 200, 64, 2), (1, 512, 64, 1)])
def test_attention_long_no_dropout_matches_reference(B, T, E, H):
    """Forward and backward against the reference model's torch maths, with the
    tolerances of test_attention_no_dropout_matches_reference, for left
    padding, a fully padded sequence and a sequence whose only valid key sits
    in the last (partial) tile."""
    torch.manual_seed(0)
    for pattern in ("left", "full", "lone"):
        qkv = torch.randn(B, T, 3 * E, device=DEV)
        ids = _ids(B, T, pattern)
        out, lse = _attn(qkv, ids, H)
        x = qkv.clone().requires_grad_(True)
        exp = _mha_reference(x, ids, H)
        print(pattern, "fwd max err", float((out - exp.detach()).abs().max()))
        assert torch.allclose(out, exp, atol=1e-5, rtol=1e-4), pattern
        g = torch.randn_like(exp)
        exp.backward(g)
        dqkv = _attn_bwd(qkv, ids, g, H, out, lse)
        print(pattern, "bwd max err", float((dqkv - x.grad).abs().max()))
        assert torch.allclose(dqkv, x.grad, atol=1e-4, rtol=1e-3), pattern


def test_attention_long_dropout_matches_hash_reference():
    torch.manual_seed(1)
    B, T, E, H, rate = 2, 130, 32, 2, 0.1
    qkv = torch.randn(B, T, 3 * E, device=DEV)
    ids = torch.randint(0, 30, (B, T), device=DEV)
    step = torch.tensor([7], dtype=torch.int64, device=DEV)
    out, lse = _attn(qkv, ids, H, rate, 123, step)
    exp = torch.empty_like(out)
    ref.attention_fwd(qkv, ids, H, rate, 123, step.cpu(), 0, exp)
    assert torch.allclose(out, exp, atol=1e-5, rtol=1e-4)
    g = torch.randn_like(out)
    d = _attn_bwd(qkv, ids, g, H, out, lse, rate, 123, step)
    e = torch.empty_like(qkv)
    ref.attention_bwd(qkv, ids, g, H, rate, 123, step.cpu(), 0, e)
    assert torch.allclose(d, e, atol=1e-4, rtol=1e-3)
    # a different step draws a different mask
    step2 = torch.tensor([8], dtype=torch.int64, device=DEV)
    out2, _ = _attn(qkv, ids, H, rate, 123, step2)
    assert not torch.allclose(out, out2)
    # Dropped fraction of a no-padding batch, read off the kernel itself: with
    # V one-hot (dim d of a head marks key 8 d) out[b, i, h, d] = P~[b, h, i, 8 d],
    # which is 0 exactly where the mask dropped it (P > 0 without padding).
    dk = E // H
    keys = torch.arange(dk, device=DEV) * 8
    ids1 = torch.ones(B, T, dtype=torch.int64, device=DEV)
    q1 = qkv.clone().view(B, T, 3, H, dk)
    q1[:, :, 2] = 0.0
    q1[:, keys, 2, :, torch.arange(dk, device=DEV)] = 1.0
    q1 = q1.view(B, T, 3 * E)
    o1, _ = _attn(q1, ids1, H, rate, 123, step)
    dropped = o1.view(B, T, H, dk) == 0                                  # [b, i, h, d]
    keep = ref.attn_keep_scale(B, H, T, rate, 123, 7, DEV)[:, :, :, keys]   # [b, h, i, d]
    assert torch.equal(dropped, keep.permute(0, 2, 1, 3) == 0)
    assert 0.0 < float(dropped.float().mean()) < 2 * rate


def test_attention_long_backward_is_deterministic():
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


def test_attention_long_argument_errors_leave_device_usable():
    """Host-side checks: nothing is launched, and a valid call still passes."""
    E, H = 16, 2
    qkv = torch.randn(1, 513, 3 * E, device=DEV)
    ids = torch.ones(1, 513, dtype=torch.int64, device=DEV)
    with pytest.raises(ValueError, match="512"):
        ops.attention_fwd(qkv, ids, H, 0.0, 1, None, 0, torch.empty(1, 513, E, device=DEV),
                          lse=torch.empty(1, H, 513, device=DEV))
    qkv = torch.randn(2, 100, 3 * E, device=DEV)
    ids = torch.ones(2, 100, dtype=torch.int64, device=DEV)
    out = torch.empty(2, 100, E, device=DEV)
    with pytest.raises(ValueError, match="lse"):
        ops.attention_fwd(qkv, ids, H, 0.0, 1, None, 0, out)
    with pytest.raises(ValueError, match="lse"):
        ops.attention_bwd(qkv, ids, out, H, 0.0, 1, None, 0, torch.empty_like(qkv))
    with pytest.raises(ValueError, match="d_k"):             # d_k = 2
        ops.attention_fwd(qkv, ids, 8, 0.0, 1, None, 0, out,
                          lse=torch.empty(2, 8, 100, device=DEV))
    got, _ = _attn(qkv, ids, H)
    assert torch.allclose(got, _mha_reference(qkv, ids, H), atol=1e-5, rtol=1e-4)


# (4, 1025): first size past the narrow path; (16, 3200): T = 50, E = 64;
# (3, 12800): T = 200, E = 64; (2, 32768): the maximum
WIDE = [(4, 1025), (16, 3200), (3, 12800), (2, 32768)]


@pytest.mark.parametrize("M,n", WIDE)
def test_layernorm_wide_fwd_bwd(M, n):
    torch.manual_seed(2)
    x = torch.randn(M, n, device=DEV) * 3 + 1
    gamma = torch.randn(n, device=DEV)
    beta = torch.randn(n, device=DEV)
    y = torch.empty_like(x)
    mean = torch.empty(M, device=DEV)
    rstd = torch.empty(M, device=DEV)
    ops.layernorm_fwd(x, n, 1e-5, gamma, beta, y, mean, rstd)
    xr = x.clone().requires_grad_(True)
    gr = gamma.clone().requires_grad_(True)
    br = beta.clone().requires_grad_(True)
    exp = torch.nn.functional.layer_norm(xr, (n,), gr, br, 1e-5)
    assert torch.allclose(y, exp, atol=1e-4, rtol=1e-4)
    g = torch.randn_like(x)
    exp.backward(g)
    dx = torch.empty_like(x)
    part = torch.empty(ops.layernorm_parts(M, n) * 2 * n, device=DEV)
    dgb = torch.empty(2 * n, device=DEV)
    ops.layernorm_bwd(x, g, n, gamma, mean, rstd, dx, part, dgb)
    assert torch.allclose(dx, xr.grad, atol=1e-4, rtol=1e-3)
    assert torch.allclose(dgb[:n], gr.grad, atol=1e-3, rtol=1e-3)
    assert torch.allclose(dgb[n:], br.grad, atol=1e-3, rtol=1e-3)


@pytest.mark.parametrize("rate", [0.0, 0.1])
@pytest.mark.parametrize("M,n", WIDE)
def test_seq_prologue_wide_fwd_bwd(M, n, rate):
    """Wide dropout(LN(x + pos)) vs the fp32 reference (same hash mask) and,
    at rate 0, vs torch autograd of the unfused ops."""
    torch.manual_seed(4)
    x = torch.randn(M, n, device=DEV) * 2 + 0.5
    pos = torch.randn(n, device=DEV)
    gamma, beta = torch.randn(n, device=DEV), torch.randn(n, device=DEV)
    step = torch.tensor([7], dtype=torch.int64, device=DEV)
    y, mean, rstd = torch.empty_like(x), torch.empty(M, device=DEV), torch.empty(M, device=DEV)
    ops.seq_prologue_fwd(x, pos, n, 1e-5, gamma, beta, rate, 1234, step, y, mean, rstd)
    ey, em, er = torch.empty_like(x), torch.empty(M, device=DEV), torch.empty(M, device=DEV)
    ref.seq_prologue_fwd(x, pos, n, 1e-5, gamma, beta, rate, 1234, step, ey, em, er)
    assert torch.allclose(y, ey, atol=1e-4, rtol=1e-4)
    g = torch.randn_like(x)
    dx = torch.empty_like(x)
    part = torch.empty(ops.layernorm_parts(M, n) * 3 * n, device=DEV)
    out3 = torch.empty(3 * n, device=DEV)
    ops.seq_prologue_bwd(x, pos, g, n, gamma, mean, rstd, rate, 1234, step, dx, part, out3)
    edx, eo3 = torch.empty_like(x), torch.empty(3 * n, device=DEV)
    ref.seq_prologue_bwd(x, pos, g, n, gamma, em, er, rate, 1234, step, edx, eo3)
    assert torch.allclose(dx, edx, atol=1e-4, rtol=1e-3)
    assert torch.allclose(out3, eo3, atol=2e-3, rtol=1e-3)
    if rate > 0:
        assert 0.0 < float((y == 0).float().mean()) < 2 * rate
        return
    xr, pr = x.clone().requires_grad_(True), pos.clone().requires_grad_(True)
    gr, br = gamma.clone().requires_grad_(True), beta.clone().requires_grad_(True)
    e = torch.nn.functional.layer_norm(xr + pr, (n,), gr, br, 1e-5)
    e.backward(g)
    assert torch.allclose(dx, xr.grad, atol=1e-4, rtol=1e-3)
    assert torch.allclose(out3[:n], gr.grad, atol=2e-3, rtol=1e-3)
    assert torch.allclose(out3[n:2 * n], br.grad, atol=2e-3, rtol=1e-3)
    assert torch.allclose(out3[2 * n:], pr.grad, atol=2e-3, rtol=1e-3)


def test_seq_prologue_wide_gidx_writes_through():
    """[dgamma | dbeta | dpos][j] lands at flat[gidx[j]] (overwriting what was
    there) and nothing else of the flat buffer is touched."""
    torch.manual_seed(5)
    M, n, rate = 5, 3200, 0.1
    x = torch.randn(M, n, device=DEV)
    pos, gamma, beta = (torch.randn(n, device=DEV) for _ in range(3))
    step = torch.tensor([2], dtype=torch.int64, device=DEV)
    y, mean, rstd = torch.empty_like(x), torch.empty(M, device=DEV), torch.empty(M, device=DEV)
    ops.seq_prologue_fwd(x, pos, n, 1e-5, gamma, beta, rate, 99, step, y, mean, rstd)
    g = torch.randn_like(x)
    part = torch.empty(0, device=DEV)
    dx, out3 = torch.empty_like(x), torch.empty(3 * n, device=DEV)
    ops.seq_prologue_bwd(x, pos, g, n, gamma, mean, rstd, rate, 99, step, dx, part, out3)
    gidx = (torch.randperm(4 * n, device=DEV)[: 3 * n] + 17).contiguous()
    flat = torch.full((4 * n + 50,), 123.0, device=DEV)
    dx2 = torch.empty_like(x)
    ops.seq_prologue_bwd(x, pos, g, n, gamma, mean, rstd, rate, 99, step, dx2, part, flat,
                         gidx=gidx)
    assert torch.equal(dx, dx2)
    assert torch.equal(flat[gidx], out3)
    untouched = torch.ones_like(flat, dtype=torch.bool)
    untouched[gidx] = False
    assert bool((flat[untouched] == 123.0).all())


@pytest.mark.parametrize("E", [32, 64])
@pytest.mark.parametrize("V,N", [(10, 7), (1000, 320), (4099, 1030)])
def test_linear_xent_wide_matches_reference(V, N, E):
    """Linear + label-smoothed CE at hidden 32 / 64 (linear_xent_wide.hip) vs
    the fp32 reference, with test_linear_xent_kernel_matches_reference's bound;
    the fused Adam step equals wgrad + the flat optimizer, bit for bit."""
    torch.manual_seed(N + E)
    H = torch.randn(N, E, device=DEV)
    W = torch.randn(V, E, device=DEV) * 0.2
    b = torch.randn(V, device=DEV) * 0.1
    y = torch.randint(1, V, (N,), device=DEV)
    y[torch.rand(N, device=DEV) < 0.6] = 0
    out = [torch.zeros(N, E, device=DEV), torch.zeros(N, device=DEV),
           torch.zeros(V, E, device=DEV), torch.zeros(V, device=DEV)]
    loss, acc = torch.zeros(1, device=DEV), torch.zeros(1, dtype=torch.float64, device=DEV)
    ops.linear_xent(H, W, b, y, 0.1, 0, *out, loss=loss, loss_acc=acc)
    exp = [torch.zeros(N, E), torch.zeros(N), torch.zeros(V, E), torch.zeros(V)]
    ops.reference.linear_xent(H.cpu(), W.cpu(), b.cpu(), y.cpu(), 0.1, 0, *exp)
    for name, a, r in zip(("dH", "loss", "dW", "db"), out, exp):
        err = float((a.cpu() - r).abs().max() / (r.abs().max() + 1e-12))
        assert err < 2e-4, (name, err)
    mean = float(exp[1].sum() / max(1, int((y != 0).sum())))
    assert abs(float(loss) - mean) < 2e-4 * max(1.0, abs(mean)) and float(acc) == float(loss)
    # fused step
    pad = -(-V // 64) * 64                    # flat-buffer padding (optim/flat.py ALIGN)
    mom = [torch.rand(V * E, device=DEV), torch.rand(V * E, device=DEV),
           torch.rand(pad, device=DEV), torch.rand(pad, device=DEV)]
    hyper = torch.tensor([1e-3, 7.0, 1.0], device=DEV)
    prm = (0.9, 0.999, 1e-8, 1e-2)
    Wa, ba = W.clone(), torch.zeros(pad, device=DEV)
    ba[:V] = b
    ma = [m.clone() for m in mom]
    dW, db = torch.zeros(V, E, device=DEV), torch.zeros(pad, device=DEV)
    ops.linear_xent(H, Wa, ba[:V], y, 0.1, 0, out[0], out[1], dW, db[:V])
    ops.dense_optimizer(Wa.view(-1), dW.view(-1), ma[0], ma[1], None, ops.OPT_ADAM, hyper, *prm)
    ops.dense_optimizer(ba, db, ma[2], ma[3], None, ops.OPT_ADAM, hyper, *prm)
    Wb, bb = W.clone(), torch.zeros(pad, device=DEV)
    bb[:V] = b
    mb = [m.clone() for m in mom]
    ops.linear_xent(H, Wb, bb[:V], y, 0.1, 0, torch.zeros(N, E, device=DEV),
                    torch.zeros(N, device=DEV), torch.zeros(V, E, device=DEV),
                    torch.zeros(pad, device=DEV)[:V],
                    step=(ops.OPT_ADAM, [mb[0], mb[1], mb[2][:V], mb[3][:V]], hyper, *prm))
    assert torch.equal(Wa, Wb) and torch.equal(ba[:V], bb[:V])
    assert torch.equal(ma[0], mb[0]) and torch.equal(ma[2][:V], mb[2][:V])


def test_bert4rec_long_encoder_matches_torch_path():
    """Whole encoder fwd + bwd at the paper shape (T = 200, hidden 64): HIP
    per-op path vs the torch reference path (dropout 0)."""
    from tdfo_amd.models import bert4rec as m

    torch.manual_seed(3)
    model = m.Bert4Rec(1000, 200, 64, 2, 2, dropout=0.0).to(DEV)
    seqs = torch.randint(0, 1000, (4, 200), device=DEV)
    seqs[:, :50] = 0
    emb = torch.randn(4, 200, 64, device=DEV, requires_grad=True)
    grads = []
    outs = []
    try:
        for fused in (True, False):
            m.USE_FUSED = fused
            model.zero_grad()
            emb.grad = None
            h = model.encode(emb, seqs)
            h.square().sum().backward()
            outs.append(h.detach())
            grads.append([emb.grad.clone()] + [p.grad.clone() for p in model.parameters()
                                               if p.grad is not None])
    finally:
        m.USE_FUSED = True
    assert torch.allclose(outs[0], outs[1], atol=1e-4, rtol=1e-4)
    assert len(grads[0]) == len(grads[1])
    for a, b in zip(grads[0], grads[1]):
        assert torch.allclose(a, b, atol=1e-3, rtol=1e-3), float((a - b).abs().max())


@pytest.mark.parametrize("T,E,H,L,B", [(50, 64, 2, 2, 8), (200, 64, 2, 1, 4)])
def test_bert4rec_long_gpu_matches_cpu(T, E, H, L, B):
    """The trainer on the per-op path (fused block off at these shapes, the
    prologue still writing through the flat gradient buffer) against the CPU
    trainer, as test_bert4rec_gpu_matches_cpu."""
    from tdfo_amd.models.bert4rec import Bert4RecTrainer

    n = 300
    kw = dict(lr=3e-3, dropout=0.0, seed=3)
    gpu = Bert4RecTrainer(n, T, E, H, L, B, device=DEV, **kw)
    cpu = Bert4RecTrainer(n, T, E, H, L, B, device="cpu", **kw)
    cpu.item.store.weight.copy_(gpu.item.store.weight.cpu())
    cpu.opt.flat.copy_(gpu.opt.flat.cpu())
    g = torch.Generator().manual_seed(0)
    for _ in range(5):
        s, l = _batch(g, B, T, n)
        gpu.load_batch(s.to(DEV), l.to(DEV))
        cpu.load_batch(s, l)
        gpu.step()
        cpu.step()
    torch.cuda.synchronize()
    assert abs(gpu.pop_loss() - cpu.pop_loss()) < 1e-3
    torch.testing.assert_close(gpu.opt.flat.cpu(), cpu.opt.flat, rtol=1e-3, atol=1e-4)
    torch.testing.assert_close(gpu.item.weight.cpu(), cpu.item.weight, rtol=1e-3, atol=1e-4)


def test_bert4rec_long_graph_replay_matches_eager():
    from tdfo_amd.models.bert4rec import Bert4RecTrainer

    n, T, E, H, L, B = 5000, 100, 32, 4, 2, 4
    kw = dict(lr=3e-3, dropout=0.0, seed=3)
    a = Bert4RecTrainer(n, T, E, H, L, B, device=DEV, **kw)
    b = Bert4RecTrainer(n, T, E, H, L, B, device=DEV, **kw)
    g = torch.Generator().manual_seed(0)
    s, l = _batch(g, B, T, n)
    for t in (a, b):
        t.load_batch(s.to(DEV), l.to(DEV))
    b.capture_graph(warmup=2)
    for _ in range(2):           # capture warmup trained b for 2 steps (capture itself does not run)
        a.step()
    for _ in range(5):
        s, l = _batch(g, B, T, n)
        for t in (a, b):
            t.load_batch(s.to(DEV), l.to(DEV))
            t.step()
    torch.cuda.synchronize()
    torch.testing.assert_close(a.opt.flat, b.opt.flat, rtol=1e-5, atol=1e-6)
    torch.testing.assert_close(a.item.weight, b.item.weight, rtol=1e-5, atol=1e-6)


def test_bert4rec_long_full_eval_and_recommend():
    from tdfo_amd.models.bert4rec import Bert4RecTrainer

    n, T, B = 400, 100, 6
    tr = Bert4RecTrainer(n, T, 32, 4, 2, B, device=DEV, dropout=0.0, seed=1)
    g = torch.Generator().manual_seed(4)
    seqs, labels = _batch(g, B, T, n)
    seqs = seqs.to(DEV)
    seqs[:, : T // 4] = 0
    targets = labels[:, -1].to(DEV)
    rank = tr.eval_batch_full(seqs, targets)
    assert rank.shape == (B,) and bool(((rank >= 0) & (rank < n)).all())
    assert set(tr.pop_metrics_full()) == {"Recall@10", "Recall@20", "Recall@50",
                                          "NDCG@10", "NDCG@20", "NDCG@50"}
    ids, scores = tr.recommend(seqs, 10)
    assert ids.shape == (B, 10) and bool(((ids >= 1) & (ids <= n)).all())
    assert not bool((ids[:, :, None] == seqs[:, None, :]).any())
    assert bool((scores[:, 1:] <= scores[:, :-1]).all())
