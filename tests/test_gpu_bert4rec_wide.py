"""The Bert4Rec trainer at hidden 128 / 256 on MI355X: the f32-MFMA output
layer (linear_xent_mfma.hip), capture, the retrieval fallback and the shape
refusals."""
import pytest
import torch

from tdfo_amd import ops
from tdfo_amd.models.bert4rec import Bert4RecTrainer
from tests.test_bert4rec import _batch

pytestmark = pytest.mark.gpu
DEV = "cuda"
N_ITEMS = 300


@pytest.fixture(scope="module", autouse=True)
def _native():
    from tdfo_amd.ops import _ext

    assert _ext.load(), "native library must load on the GPU box"


@pytest.mark.parametrize("E,heads,T,steps", [(128, 2, 20, 5), (256, 4, 20, 1), (128, 2, 100, 1)])
def test_bert4rec_wide_gpu_matches_cpu(E, heads, T, steps):
    """Steps from copied weights, the tolerances of
    test_bert4rec_gpu_matches_cpu; T = 100 takes the tiled attention and the
    wide LayerNorm (n = 12800).

    (128, 2, 20) runs the 5 steps. The other two miss the parameter tolerance
    after more than one step, and they miss it the same way with the output
    layer swapped for eager F.cross_entropy on materialised logits, so the
    drift is the encoder's, not the output kernel's (measured on MI355X, max
    |GPU - CPU| over the flat parameters, fused output / eager output):
      (256, 4, 20): step 1 1.3e-4 / 1.0e-4 (both hold), step 2 7.2e-4 / 7.2e-4
                    (22 elements out, both), step 5 7.6e-3 / 7.6e-3 (4940 out)
      (128, 2, 100): step 1 9.9e-5 (holds) / 1.9e-4 (1 element out), step 5
                    2.8e-4 / 2.5e-4 (1 / 2 elements of 473920 out)
    (Adam divides a gradient that is rounding noise by its own magnitude.) They
    are cut to 1 step; profiles/wide_hidden.md has the whole table."""
    n, B = N_ITEMS, 16
    kw = dict(lr=3e-3, dropout=0.0, seed=3)
    gpu = Bert4RecTrainer(n, T, E, heads, 2, B, device=DEV, **kw)
    cpu = Bert4RecTrainer(n, T, E, heads, 2, B, device="cpu", **kw)
    cpu.item.store.weight.copy_(gpu.item.store.weight.cpu())
    cpu.opt.flat.copy_(gpu.opt.flat.cpu())
    g = torch.Generator().manual_seed(0)
    for _ in range(steps):
        s, l = _batch(g, B, T, n)
        gpu.load_batch(s.to(DEV), l.to(DEV))
        cpu.load_batch(s, l)
        gpu.step()
        cpu.step()
    torch.cuda.synchronize()
    lg, lc = gpu.pop_loss(), cpu.pop_loss()
    dflat = float((gpu.opt.flat.cpu() - cpu.opt.flat).abs().max())
    ditem = float((gpu.item.weight.cpu() - cpu.item.weight).abs().max())
    print(f"E={E} heads={heads} T={T}: loss gpu {lg:.6f} cpu {lc:.6f}; max |d flat| {dflat:.3e}, "
          f"max |d item| {ditem:.3e}")
    assert abs(lg - lc) < 1e-3
    torch.testing.assert_close(gpu.opt.flat.cpu(), cpu.opt.flat, rtol=1e-3, atol=1e-4)
    torch.testing.assert_close(gpu.item.weight.cpu(), cpu.item.weight, rtol=1e-3, atol=1e-4)


def test_bert4rec_wide_graph_replay_same_bits():
    """At (128, 2, 20) the captured step gives the bits of the eager step."""
    n, T, B = N_ITEMS, 20, 16
    kw = dict(lr=3e-3, dropout=0.0, seed=3)
    a = Bert4RecTrainer(n, T, 128, 2, 2, B, device=DEV, **kw)
    b = Bert4RecTrainer(n, T, 128, 2, 2, B, device=DEV, **kw)
    g = torch.Generator().manual_seed(0)
    s, l = _batch(g, B, T, n)
    for t in (a, b):
        t.load_batch(s.to(DEV), l.to(DEV))
    b.capture_graph(warmup=2)
    assert b.graph is not None
    for _ in range(2):           # the capture warm-up trained b for 2 steps
        a.step()
    for _ in range(3):
        s, l = _batch(g, B, T, n)
        for t in (a, b):
            t.load_batch(s.to(DEV), l.to(DEV))
            t.step()
    torch.cuda.synchronize()
    assert torch.equal(a.opt.flat, b.opt.flat)
    assert torch.equal(a.item.weight, b.item.weight)
    assert torch.equal(a.model.out.weight, b.model.out.weight)


def test_bert4rec_wide_same_seed_same_bits():
    """Two trainers with one seed end bit-identical with dropout 0.1. They run
    one after the other: at this width the encoder takes the per-op path,
    whose nn.Dropout draws from torch's generator, which the constructor
    seeds."""
    n, T, B = N_ITEMS, 20, 16
    kw = dict(lr=3e-3, dropout=0.1, seed=11)
    done = []
    for _ in range(2):
        t = Bert4RecTrainer(n, T, 128, 2, 2, B, device=DEV, **kw)
        g = torch.Generator().manual_seed(2)
        for _ in range(3):
            s, l = _batch(g, B, T, n)
            t.load_batch(s.to(DEV), l.to(DEV))
            t.step()
        done.append(t)
    a, b = done
    torch.cuda.synchronize()
    assert torch.equal(a.opt.flat, b.opt.flat)
    assert torch.equal(a.item.weight, b.item.weight)
    assert a.pop_loss() == b.pop_loss()


def test_bert4rec_wide_retrieval_fallback():
    """recommend / eval_batch_full at E = 128: the chunked reference on the
    device, equal to the reference on CPU copies of the same hidden states."""
    n, T, B = N_ITEMS, 20, 8
    tr = Bert4RecTrainer(n, T, 128, 2, 2, B, device=DEV, dropout=0.0, seed=4)
    g = torch.Generator().manual_seed(1)
    seqs = torch.randint(1, n + 1, (B, T), generator=g)
    seqs[0, :5] = 0                                          # left padding
    seqs[:, -1] = n + 1                                      # MASK at the predicted position
    seqs = seqs.to(DEV)
    W, bias = tr.model.out.weight.detach(), tr.model.out.bias.detach()
    h = tr._last_hidden(seqs)
    assert h.shape == (B, 128)
    for seen in (True, False):
        ids, scores = tr.recommend(seqs, 10, exclude_seen=seen)
        ri = torch.empty(B, 10, dtype=torch.int64)
        rs = torch.empty(B, 10, dtype=torch.float32)
        ops.reference.topk_scores(h.cpu(), W.cpu(), bias.cpu(), 10, ri, rs, 1, tr.V - 1,
                                  exclude=seqs.cpu() if seen else None)
        assert torch.equal(ids.cpu(), ri)
        torch.testing.assert_close(scores.cpu(), rs)
        got = ids.cpu()
        assert bool((got >= 1).all()) and bool((got <= n).all())
        if seen:
            for r in range(B):
                assert not set(got[r].tolist()) & set(seqs[r].tolist())
    targets = torch.randint(1, n + 1, (B,), generator=g).to(DEV)
    rank = tr.eval_batch_full(seqs, targets)
    assert rank.shape == (B,) and bool((rank >= 0).all()) and bool((rank < n).all())
    m = tr.pop_metrics_full()
    assert all(0.0 <= v <= 1.0 for v in m.values())


@pytest.mark.parametrize("E,heads,T", [(128, 1, 20), (256, 2, 20), (256, 4, 200), (96, 2, 20)])
def test_bert4rec_wide_shape_refusals(E, heads, T):
    """d_k = 128, T * E over 32768 and hidden 96 are refused at construction,
    by one ValueError that names the supported set."""
    with pytest.raises(ValueError, match=r"\(16, 32, 64, 128, 256\)"):
        Bert4RecTrainer(N_ITEMS, T, E, heads, 2, 16, device=DEV)
