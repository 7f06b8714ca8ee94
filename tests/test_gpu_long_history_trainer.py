"""Bert4Rec / the next-item trainer at max_len above 512 on MI355X: the
per-op encoder on the streaming attention kernels (attention_stream.hip)
against the CPU trainer, with the full and the BCE loss, causal and not;
no-leak; capture; the shape check's new maximum. Built like
tests/test_gpu_sasrec.py, with its tolerances."""
import pytest
import torch

from tdfo_amd import ops
from tdfo_amd.models.bert4rec import Bert4Rec, Bert4RecTrainer
from tests.test_sasrec import _next_item_batch

pytestmark = pytest.mark.gpu
DEV = "cuda"
N_ITEMS = 300
DATA_SEED = 1


@pytest.fixture(scope="module", autouse=True)
def _native():
    from tdfo_amd.ops import _ext

    assert _ext.load(), "native library must load on the GPU box"


def _pair(E, heads, T, B, causal=True, **kw):
    gpu = Bert4RecTrainer(N_ITEMS, T, E, heads, 2, B, device=DEV, causal=causal, **kw)
    cpu = Bert4RecTrainer(N_ITEMS, T, E, heads, 2, B, device="cpu", causal=causal, **kw)
    cpu.item.store.weight.copy_(gpu.item.store.weight.cpu())
    cpu.opt.flat.copy_(gpu.opt.flat.cpu())
    return gpu, cpu


def _masked_batch(g, B, T):
    s = torch.randint(1, N_ITEMS + 1, (B, T), generator=g)
    m = torch.rand(B, T, generator=g) < 0.2
    m[:, -1] = True
    return torch.where(m, torch.full_like(s, N_ITEMS + 1), s), torch.where(m, s, torch.zeros_like(s))


def _one_step_matches(gpu, cpu, batch, tag):
    s, l = batch
    gpu.load_batch(s.to(DEV), l.to(DEV))
    cpu.load_batch(s, l)
    gpu.step()
    cpu.step()
    torch.cuda.synchronize()
    lg, lc = gpu.pop_loss(), cpu.pop_loss()
    dflat = float((gpu.opt.flat.cpu() - cpu.opt.flat).abs().max())
    ditem = float((gpu.item.weight.cpu() - cpu.item.weight).abs().max())
    print(f"{tag}: loss gpu {lg:.6f} cpu {lc:.6f}; max |d flat| {dflat:.3e}, "
          f"max |d item| {ditem:.3e}")
    assert abs(lg - lc) < 1e-3
    torch.testing.assert_close(gpu.opt.flat.cpu(), cpu.opt.flat, rtol=1e-3, atol=1e-4)
    torch.testing.assert_close(gpu.item.weight.cpu(), cpu.item.weight, rtol=1e-3, atol=1e-4)


@pytest.mark.parametrize("E,heads,T,B", [(16, 2, 576, 4), (64, 1, 1025, 2)])
def test_long_history_gpu_matches_cpu(E, heads, T, B):
    assert T > ops.ATTN_LONG_MAXT
    gpu, cpu = _pair(E, heads, T, B, lr=3e-3, dropout=0.0, seed=3)
    g = torch.Generator().manual_seed(DATA_SEED)
    _one_step_matches(gpu, cpu, _next_item_batch(g, B, T, N_ITEMS), f"E={E} heads={heads} T={T}")


def test_long_history_bce_gpu_matches_cpu():
    E, heads, T, B = 16, 2, 640, 2
    gpu, cpu = _pair(E, heads, T, B, lr=3e-3, dropout=0.0, seed=3, loss="bce", num_negatives=64)
    g = torch.Generator().manual_seed(DATA_SEED)
    _one_step_matches(gpu, cpu, _next_item_batch(g, B, T, N_ITEMS), f"bce E={E} T={T}")
    assert torch.equal(gpu.negs.cpu(), cpu.negs)


def test_long_history_non_causal_gpu_matches_cpu():
    """masked-item Bert4Rec at max_len 1024: the joint [T, E] row is 16384"""
    E, heads, T, B = 16, 2, 1024, 2
    gpu, cpu = _pair(E, heads, T, B, causal=False, lr=3e-3, dropout=0.0, seed=3)
    g = torch.Generator().manual_seed(DATA_SEED)
    _one_step_matches(gpu, cpu, _masked_batch(g, B, T), f"non-causal E={E} T={T}")


def test_long_history_model_no_leak_on_gpu():
    torch.manual_seed(0)
    B, E, T = 3, 16, 700
    model = Bert4Rec(N_ITEMS + 2, T, E, 2, 2, dropout=0.1, causal=True).to(DEV).eval()
    table = torch.randn(N_ITEMS + 2, E, device=DEV)
    seqs = torch.randint(1, N_ITEMS, (B, T), device=DEV)
    seqs[0, : T // 4] = 0
    with torch.no_grad():
        base = model.encode(table[seqs], seqs)
        for t in (0, 511, 512, T - 2):
            other = seqs.clone()
            other[:, t + 1:] = torch.randint(0, N_ITEMS, (B, T - t - 1), device=DEV)
            got = model.encode(table[other], other)
            assert torch.equal(got[:, : t + 1], base[:, : t + 1]), t
            assert not torch.equal(got[:, t + 1:], base[:, t + 1:])


def test_long_history_graph_replay_same_bits():
    """a captured step at max_len 576 gives the bits of the eager step"""
    T, B = 576, 2
    kw = dict(lr=3e-3, dropout=0.0, seed=3, causal=True)
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
    for _ in range(3):
        s, l = _next_item_batch(g, B, T, N_ITEMS)
        for t in (a, b):
            t.load_batch(s.to(DEV), l.to(DEV))
            t.step()
    torch.cuda.synchronize()
    assert torch.equal(a.opt.flat, b.opt.flat)
    assert torch.equal(a.item.weight, b.item.weight)
    assert torch.equal(a.model.out.weight, b.model.out.weight)


def test_long_history_shape_check():
    tr = Bert4RecTrainer(N_ITEMS, 4096, 64, 1, 1, 1, device=DEV, causal=True)
    assert tr.T == 4096
    with pytest.raises(ValueError, match="4096"):
        Bert4RecTrainer(N_ITEMS, 4097, 64, 1, 1, 1, device=DEV, causal=True)
    with pytest.raises(ValueError, match=r"\(16, 32, 64, 128, 256\)"):
        Bert4RecTrainer(N_ITEMS, 1024, 64, 2, 1, 2, device=DEV)          # 1024 * 64 > 32768
