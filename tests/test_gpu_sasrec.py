"""The causal (next-item) Bert4Rec trainer on MI355X: per-op encoder with the
causal attention kernels and the per-position input block, against the CPU
trainer; capture; no-leak; retrieval; the shape check."""
import pytest
import torch

from tdfo_amd import ops
from tdfo_amd.models.bert4rec import Bert4Rec, Bert4RecTrainer
from tests.test_sasrec import _next_item_batch

pytestmark = pytest.mark.gpu
DEV = "cuda"
N_ITEMS = 300


@pytest.fixture(scope="module", autouse=True)
def _native():
    from tdfo_amd.ops import _ext

    assert _ext.load(), "native library must load on the GPU box"


def _pair(E, heads, T, B, **kw):
    gpu = Bert4RecTrainer(N_ITEMS, T, E, heads, 2, B, device=DEV, causal=True, **kw)
    cpu = Bert4RecTrainer(N_ITEMS, T, E, heads, 2, B, device="cpu", causal=True, **kw)
    cpu.item.store.weight.copy_(gpu.item.store.weight.cpu())
    cpu.opt.flat.copy_(gpu.opt.flat.cpu())
    return gpu, cpu


# Generator seed of the batches. Seed 0 puts the comparison on an ill-conditioned
# point at (16, 2, 20): for one element of block 1's feed_forward.w_2.weight the
# gradient (2.0325e-6 on the CPU, 2.0309e-6 on the GPU) cancels against the L2
# decay term wd p (-2.03e-6) to a few 1e-9, below Adam's eps = 1e-8, where the
# first update lr g' / (|g'| + eps) turns that 8e-4 relative gradient difference
# into 4.6e-4 of parameter (1 of 13056 elements out from step 1 on, every other
# within 7e-5, no growth over 5 steps; the same element misses by 4.3e-4 with
# the torch ops on the same GPU in place of the HIP kernels, so it is the
# comparison's conditioning, not the kernels). (64, 2, 100) and (128, 2, 20)
# held for 5 steps with seed 0 (max |d flat| 5.6e-5 / 9.9e-5).
DATA_SEED = 1


@pytest.mark.parametrize("E,heads,T,steps", [(16, 2, 20, 5), (64, 2, 100, 1), (128, 2, 20, 1)])
def test_sasrec_gpu_matches_cpu(E, heads, T, steps):
    """Steps from copied weights on next-item batches (labels = the next item,
    right-padded tails), the tolerances of test_bert4rec_wide_gpu_matches_cpu."""
    B = 16
    gpu, cpu = _pair(E, heads, T, B, lr=3e-3, dropout=0.0, seed=3)
    g = torch.Generator().manual_seed(DATA_SEED)
    for _ in range(steps):
        s, l = _next_item_batch(g, B, T, N_ITEMS)
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


def test_sasrec_graph_replay_same_bits():
    """At (16, 2, 20) -- where a non-causal trainer takes the fused block and
    zeroes only the uncovered gradient ranges -- the captured causal step gives
    the bits of the eager step: every gradient is zeroed each step."""
    T, B = 20, 16
    kw = dict(lr=3e-3, dropout=0.0, seed=3, causal=True)
    a = Bert4RecTrainer(N_ITEMS, T, 16, 2, 2, B, device=DEV, **kw)
    b = Bert4RecTrainer(N_ITEMS, T, 16, 2, 2, B, device=DEV, **kw)
    assert a._zero_ranges is None and getattr(a.model, "gdst", None) is None
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


@pytest.mark.parametrize("E,T", [(16, 20), (64, 100)])
def test_sasrec_model_no_leak_on_gpu(E, T):
    torch.manual_seed(0)
    B = 3
    model = Bert4Rec(N_ITEMS + 2, T, E, 2, 2, dropout=0.1, causal=True).to(DEV).eval()
    table = torch.randn(N_ITEMS + 2, E, device=DEV)
    seqs = torch.randint(1, N_ITEMS, (B, T), device=DEV)
    seqs[0, : T // 4] = 0
    with torch.no_grad():
        base = model.encode(table[seqs], seqs)
        for t in (0, T // 4, T // 2, min(T - 2, 64), T - 2):
            other = seqs.clone()
            other[:, t + 1:] = torch.randint(0, N_ITEMS, (B, T - t - 1), device=DEV)
            got = model.encode(table[other], other)
            assert torch.equal(got[:, : t + 1], base[:, : t + 1]), t
            assert not torch.equal(got[:, t + 1:], base[:, t + 1:])


def _retrieval_case(seed, B=32, T=20, k=10):
    """CPU side of the retrieval test: a causal CPU trainer, left-padded
    histories, the reference top-(k + 1) and ranks, and which rows have score
    gaps above 1e-4 (so that fp32 rounding cannot reorder them)."""
    cpu = Bert4RecTrainer(N_ITEMS, T, 16, 2, 2, B, device="cpu", dropout=0.0, seed=seed,
                          causal=True)
    g = torch.Generator().manual_seed(seed)
    seqs = torch.randint(1, N_ITEMS + 1, (B, T), generator=g)
    pad = torch.randint(0, T - 1, (B, 1), generator=g)
    seqs = torch.where(torch.arange(T)[None, :] < pad, torch.zeros_like(seqs), seqs)
    targets = torch.randint(1, N_ITEMS + 1, (B,), generator=g)
    with torch.no_grad():
        h = cpu._last_hidden(seqs)
        W, bias = cpu.model.out.weight.detach(), cpu.model.out.bias.detach()
        ri = torch.empty(B, k + 1, dtype=torch.int64)
        rs = torch.empty(B, k + 1, dtype=torch.float32)
        ops.topk_scores(h, W, bias, k + 1, ri, rs, 1, cpu.V - 1, exclude=seqs)
        rank = torch.empty(B, dtype=torch.int64)
        one_i = torch.empty(B, 1, dtype=torch.int64)
        one_s = torch.empty(B, 1, dtype=torch.float32)
        ops.topk_scores(h, W, bias, 1, one_i, one_s, 1, cpu.V - 1, target=targets, out_rank=rank)
        top_ok = (rs[:, :-1] - rs[:, 1:]).min(1).values > 1e-4
        full = h @ W[1: cpu.V - 1].t() + bias[1: cpu.V - 1]                  # items 1 .. n
        gap = (full - full.gather(1, (targets - 1)[:, None])).abs()
        gap.scatter_(1, (targets - 1)[:, None], float("inf"))
        rank_ok = gap.min(1).values > 1e-4
    return cpu, seqs, targets, ri[:, :k], rank, top_ok, rank_ok


RETRIEVAL_SEED = 5       # (CPU reference alone: 100 % / 94 % of the rows have such gaps)


def test_sasrec_retrieval_matches_cpu_reference():
    """recommend / eval_batch_full of a causal GPU trainer against
    ops.topk_scores on the CPU trainer's last hidden state (E = 16): exact ids
    and ranks on the rows whose reference score gaps exceed 1e-4, which must be
    at least 90 % of the rows."""
    k = 10
    cpu, seqs, targets, ri, rrank, top_ok, rank_ok = _retrieval_case(RETRIEVAL_SEED, k=k)
    B, T = seqs.shape
    assert float(top_ok.float().mean()) >= 0.9 and float(rank_ok.float().mean()) >= 0.9
    gpu = Bert4RecTrainer(N_ITEMS, T, 16, 2, 2, B, device=DEV, dropout=0.0, seed=RETRIEVAL_SEED,
                          causal=True)
    gpu.item.store.weight.copy_(cpu.item.store.weight.to(DEV))
    gpu.opt.flat.copy_(cpu.opt.flat.to(DEV))
    ids, scores = gpu.recommend(seqs.to(DEV), k)
    assert torch.equal(ids.cpu()[top_ok], ri[top_ok])
    assert bool((scores[:, 1:] <= scores[:, :-1]).all())
    rank = gpu.eval_batch_full(seqs.to(DEV), targets.to(DEV))
    assert torch.equal(rank.cpu()[rank_ok], rrank[rank_ok])
    assert all(0.0 <= v <= 1.0 for v in gpu.pop_metrics_full().values())


def test_sasrec_shape_check():
    """No joint-row limit for a causal trainer; the other limits stay."""
    tr = Bert4RecTrainer(N_ITEMS, 512, 128, 2, 1, 2, device=DEV, causal=True)
    assert tuple(tr.model.layernorm.weight.shape) == (128,)
    with pytest.raises(ValueError, match=r"\(16, 32, 64, 128, 256\)"):
        Bert4RecTrainer(N_ITEMS, 512, 128, 2, 1, 2, device=DEV)          # 512 * 128 > 32768
    with pytest.raises(ValueError, match=r"\(16, 32, 64, 128, 256\)"):
        Bert4RecTrainer(N_ITEMS, 20, 48, 2, 1, 2, device=DEV, causal=True)
