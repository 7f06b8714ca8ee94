"""Bert4RecTrainer(loss="bce") on MI355X: the BCE / gBCE step against the CPU
trainer (causal and masked), and the captured graph against eager steps."""
import pytest
import torch

from tdfo_amd.models.bert4rec import Bert4RecTrainer
from tests.test_sasrec import _next_item_batch

pytestmark = pytest.mark.gpu
DEV = "cuda"
N_ITEMS, S, B = 300, 64, 16
DATA_SEED = 1


@pytest.fixture(scope="module", autouse=True)
def _native():
    from tdfo_amd.ops import _ext

    assert _ext.load(), "native library must load on the GPU box"


def _pair(E, heads, T, causal, t):
    kw = dict(lr=3e-3, dropout=0.0, seed=3, causal=causal, loss="bce", num_negatives=S, gbce_t=t)
    gpu = Bert4RecTrainer(N_ITEMS, T, E, heads, 2, B, device=DEV, **kw)
    cpu = Bert4RecTrainer(N_ITEMS, T, E, heads, 2, B, device="cpu", **kw)
    cpu.item.store.weight.copy_(gpu.item.store.weight.cpu())
    cpu.opt.flat.copy_(gpu.opt.flat.cpu())
    return gpu, cpu


def _masked_batch(g, T):
    s = torch.randint(1, N_ITEMS + 1, (B, T), generator=g)
    m = torch.rand(B, T, generator=g) < 0.2
    m[:, -1] = True
    return torch.where(m, torch.full_like(s, N_ITEMS + 1), s), torch.where(m, s, torch.zeros_like(s))


@pytest.mark.parametrize("E,heads,T,steps,causal,t",
                         [(16, 2, 20, 3, True, 0.0), (64, 2, 100, 1, True, 0.75),
                          (128, 2, 20, 1, True, 0.75), (16, 2, 20, 1, False, 0.75)])
def test_bce_gpu_matches_cpu(E, heads, T, steps, causal, t):
    """Steps from copied weights, the tolerances of test_sampled_gpu_matches_cpu
    (the encoder is the same); the negatives and the label order are equal
    exactly."""
    gpu, cpu = _pair(E, heads, T, causal, t)
    assert gpu._xent_step is None and gpu.beta == cpu.beta
    g = torch.Generator().manual_seed(DATA_SEED)
    for _ in range(steps):
        s, l = _next_item_batch(g, B, T, N_ITEMS) if causal else _masked_batch(g, T)
        gpu.load_batch(s.to(DEV), l.to(DEV))
        cpu.load_batch(s, l)
        gpu.step()
        cpu.step()
        assert torch.equal(gpu.neg.cpu(), cpu.neg)
        assert torch.equal(gpu.negs.cpu(), cpu.negs)
        assert torch.equal(gpu.order.cpu(), cpu.order)
    torch.cuda.synchronize()
    lg, lc = gpu.pop_loss(), cpu.pop_loss()
    dflat = float((gpu.opt.flat.cpu() - cpu.opt.flat).abs().max())
    ditem = float((gpu.item.weight.cpu() - cpu.item.weight).abs().max())
    print(f"E={E} heads={heads} T={T} causal={causal} t={t}: loss gpu {lg:.6f} cpu {lc:.6f}; "
          f"max |d flat| {dflat:.3e}, max |d item| {ditem:.3e}")
    assert abs(lg - lc) < 1e-3
    torch.testing.assert_close(gpu.opt.flat.cpu(), cpu.opt.flat, rtol=1e-3, atol=1e-4)
    torch.testing.assert_close(gpu.item.weight.cpu(), cpu.item.weight, rtol=1e-3, atol=1e-4)


def test_bce_graph_replay_same_bits():
    """3 replayed steps equal 3 eager steps bit for bit, and the negatives
    differ between two consecutive replays (the sampler reads the device step
    counter)."""
    T = 20
    kw = dict(lr=3e-3, dropout=0.0, seed=3, causal=True, loss="bce", num_negatives=S, gbce_t=0.75)
    a = Bert4RecTrainer(N_ITEMS, T, 16, 2, 2, B, device=DEV, **kw)
    b = Bert4RecTrainer(N_ITEMS, T, 16, 2, 2, B, device=DEV, **kw)
    g = torch.Generator().manual_seed(0)
    s, l = _next_item_batch(g, B, T, N_ITEMS)
    for t in (a, b):
        t.load_batch(s.to(DEV), l.to(DEV))
    b.capture_graph(warmup=2)
    assert b.graph is not None
    for _ in range(2):           # the capture warm-up trained b for 2 steps
        a.step()
    seen = []
    for _ in range(3):
        s, l = _next_item_batch(g, B, T, N_ITEMS)
        for t in (a, b):
            t.load_batch(s.to(DEV), l.to(DEV))
            t.step()
        assert torch.equal(a.negs, b.negs) and torch.equal(a.order, b.order)
        seen.append((b.negs.clone(), b.neg.clone()))
    torch.cuda.synchronize()
    for (c0, n0), (c1, n1) in zip(seen, seen[1:]):
        assert not torch.equal(c0, c1) and not torch.equal(n0, n1)
    assert torch.equal(a.opt.flat, b.opt.flat)
    assert torch.equal(a.item.weight, b.item.weight)
    assert torch.equal(a.model.out.weight, b.model.out.weight)
