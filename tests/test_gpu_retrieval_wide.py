"""The fused full-catalogue top-K search at E = 128 / 256 on MI355X (32
queries per block, item rows streamed in groups of chunks): the checks of
test_gpu_retrieval.py at the wide widths. Exact against the CPU reference on
integer-valued data (every sum stays below 2^24), within the fp32 chain bound
of an fp64 score matrix on random data, bit-identical across runs and V
splits, capturable, and through the Bert4Rec trainer at hidden 128 / 256."""
import pytest
import torch

from tdfo_amd import ops
from tdfo_amd.models.bert4rec import Bert4RecTrainer
from tests.retrieval_cases import exact_case, inner_range, run_topk

pytestmark = pytest.mark.gpu
DEV = "cuda"
WIDTHS = (16, 32, 64, 128, 256)


@pytest.fixture(scope="module", autouse=True)
def _native():
    from tdfo_amd.ops import _ext

    assert _ext.load(), "native library must load on the GPU box"


def _dev(t):
    return None if t is None else t.to(DEV)


def _run_case(c, with_target=True):
    out = run_topk(_dev(c["q"]), _dev(c["W"]), _dev(c["bias"]), c["K"], c["v_lo"], c["v_hi"],
                   _dev(c["exclude"]), _dev(c["target"]) if with_target else None)
    torch.cuda.synchronize()
    return [None if t is None else t.cpu() for t in out]


def test_fused_widths_and_native_op():
    """The public list of widths, and the native op itself (not ops.topk_scores,
    which could dispatch elsewhere) at both wide widths on a tiny case."""
    assert tuple(ops.topk_fused_widths()) == WIDTHS
    from tdfo_amd.ops import _native as native

    for E in (128, 256):
        c = exact_case(E, 3, 40, 5, 0)
        ids = torch.empty(3, 5, dtype=torch.int64, device=DEV)
        scores = torch.empty(3, 5, device=DEV)
        native().topk_scores(_dev(c["q"]), _dev(c["W"]), _dev(c["bias"]), 5, ids, scores,
                             c["v_lo"], c["v_hi"], None, None, None)
        torch.cuda.synchronize()
        assert torch.equal(ids.cpu(), c["ids"]) and torch.equal(scores.cpu(), c["scores"])


# (E, B, V, K, X): at either width every B in {1, 17, 33, 130} (a partial
# query tile, more than one and more than two tiles of 32 or of 64), V in
# {1, 7, 300, 4099, 100_003} (V < K, V < one item tile, a prime V, enough item
# tiles for 64 splits), K in {1, 10, 100, 128}, X in {0, 1, 20, 50}
EXACT = [
    (128, 1, 1, 1, 0), (128, 17, 7, 10, 1), (128, 33, 300, 128, 20), (128, 130, 300, 100, 50),
    (128, 130, 4099, 10, 0), (128, 33, 4099, 100, 20), (128, 17, 100_003, 128, 50),
    (128, 1, 100_003, 100, 1),
    (256, 17, 1, 10, 1), (256, 33, 7, 128, 20), (256, 1, 300, 1, 0), (256, 130, 300, 100, 50),
    (256, 17, 4099, 128, 50), (256, 130, 4099, 10, 20), (256, 33, 100_003, 100, 20),
    (256, 130, 100_003, 1, 0),
]


def test_exact_axes_covered():
    for E in (128, 256):
        for axis, want in ((1, {1, 17, 33, 130}), (2, {1, 7, 300, 4099, 100_003}),
                           (3, {1, 10, 100, 128}), (4, {0, 1, 20, 50})):
            assert {c[axis] for c in EXACT if c[0] == E} == want


@pytest.mark.parametrize("E,B,V,K,X", EXACT)
def test_exact_cases(E, B, V, K, X):
    """v_lo = 1, v_hi = V - 1, the ties, exclusions and targets of exact_case:
    ids, scores and rank equal the CPU reference exactly, with and without a
    target."""
    c = exact_case(E, B, V, K, X)
    ids, scores, rank = _run_case(c)
    assert torch.equal(ids, c["ids"])
    assert torch.equal(scores, c["scores"])
    assert torch.equal(rank, c["rank"])
    ids2, scores2, rank2 = _run_case(c, with_target=False)
    assert rank2 is None and torch.equal(ids2, ids) and torch.equal(scores2, scores)


@pytest.mark.parametrize("E,B,V,K,X", [(128, 17, 300, 10, 20), (256, 33, 4099, 128, 1)])
def test_exact_cases_whole_range(E, B, V, K, X):
    c = exact_case(E, B, V, K, X, True)
    ids, scores, rank = _run_case(c)
    assert torch.equal(ids, c["ids"]) and torch.equal(scores, c["scores"])
    assert torch.equal(rank, c["rank"])
    ids2, scores2, rank2 = _run_case(c, with_target=False)
    assert rank2 is None and torch.equal(ids2, ids) and torch.equal(scores2, scores)


@pytest.mark.parametrize("descending", [False, True])
def test_adversarial_order(descending):
    """E = 128. Query 0's scores ascend with the id: every item beats its
    threshold, the worst case for buffer compactions; or descend: none after
    the first K. Splits auto and 1."""
    g = torch.Generator().manual_seed(5)
    B, E, V, K = 17, 128, 20_011, 100
    q = torch.randint(-3, 4, (B, E), generator=g).float()
    W = torch.randint(-3, 4, (V, E), generator=g).float()
    bias = torch.randint(-2, 3, (V,), generator=g).float()
    s0 = W @ q[0] + bias
    perm = torch.sort(s0, descending=descending, stable=True).indices
    W, bias = W[perm].contiguous(), bias[perm].contiguous()
    s0 = W @ q[0] + bias
    assert bool((s0[1:] <= s0[:-1]).all() if descending else (s0[1:] >= s0[:-1]).all())
    target = torch.randint(0, V, (B,), generator=g)
    excl = torch.randint(-1, V, (B, 20), generator=g)
    c = dict(q=q, W=W, bias=bias, K=K, v_lo=1, v_hi=V - 1, exclude=excl, target=target)
    want = run_topk(q, W, bias, K, 1, V - 1, excl, target)
    for s in (0, 1):
        old = ops.topk_splits(s)
        try:
            ids, scores, rank = _run_case(c)
        finally:
            ops.topk_splits(old)
        assert torch.equal(ids, want[0]) and torch.equal(scores, want[1]), f"splits={s}"
        assert torch.equal(rank, want[2]), f"splits={s}"


@pytest.mark.parametrize("E,B,V,K,X", [(128, 33, 300, 100, 20), (256, 33, 4099, 128, 20),
                                        (128, 130, 4099, 100, 0), (256, 130, 300, 10, 50)])
def test_random_float_cases(E, B, V, K, X):
    """Against an fp64 score matrix: tol[b, v] = 2 gamma (sum_e |q w| + |bias|),
    gamma = (E+1) 2^-24 / (1 - (E+1) 2^-24), the bound of an (E+1)-term fp32
    chain in any order of summation."""
    g = torch.Generator().manual_seed(E + V + K)
    q = torch.randn(B, E, generator=g)
    W = torch.randn(V, E, generator=g)
    bias = torch.randn(V, generator=g)
    v_lo, v_hi = inner_range(V)
    excl = torch.randint(-1, V, (B, X), generator=g) if X else None
    target = torch.randint(0, V, (B,), generator=g)
    c = dict(q=q, W=W, bias=bias, K=K, v_lo=v_lo, v_hi=v_hi, exclude=excl, target=target)
    ids, scores, rank = _run_case(c)
    s64 = q.double() @ W.double().t() + bias.double()
    u = (E + 1) * 2.0 ** -24
    tol = 2 * (u / (1 - u)) * (q.double().abs() @ W.double().abs().t() + bias.double().abs())
    elig = torch.zeros(B, V, dtype=torch.bool)
    elig[:, v_lo:v_hi] = True
    if excl is not None:
        for b in range(B):
            e = excl[b][excl[b] >= 0]
            elig[b, e] = False
    n_elig = elig.sum(1)
    for b in range(B):
        n = min(K, int(n_elig[b]))
        got = ids[b, :n]
        assert (ids[b, n:] == -1).all() and (scores[b, n:] == float("-inf")).all()
        assert len(set(got.tolist())) == n and bool(elig[b, got].all())
        assert bool((scores[b, 1:n] <= scores[b, : n - 1]).all())
        assert bool(((scores[b, :n].double() - s64[b, got]).abs() <= tol[b, got]).all())
        rest = elig[b].clone()
        rest[got] = False
        if n and rest.any():
            floor = s64[b, got].min()
            assert bool((s64[b, rest] <= floor + 2 * tol[b, rest]).all())
        t = int(target[b])
        others = elig[b].clone()
        others[t] = False
        lo = int((s64[b, others] > s64[b, t] + 2 * tol[b, others]).sum())
        hi = int((s64[b, others] >= s64[b, t] - 2 * tol[b, others]).sum())
        assert lo <= int(rank[b]) <= hi


def test_deterministic_and_split_independent():
    """E = 256. Rows 0 .. 499 are scaled up, so that many of them reach the top
    K, and copied to 60_000 .. 60_499: with 2 (boundary 50_049), 7 (14_336 ids
    each) and the automatic 61 ranges of V the copy lies in another range than
    its original, so exact float ties cross range boundaries."""
    g = torch.Generator().manual_seed(11)
    B, E, V, K = 33, 256, 100_003, 100
    c = dict(q=torch.randn(B, E, generator=g), W=torch.randn(V, E, generator=g),
             bias=torch.randn(V, generator=g), K=K, v_lo=1, v_hi=V - 1,
             exclude=torch.randint(-1, V, (B, 20), generator=g),
             target=torch.randint(0, V, (B,), generator=g))
    c["W"][:500] *= 1.5
    c["W"][60_000:60_500] = c["W"][:500]
    c["bias"][60_000:60_500] = c["bias"][:500]
    base = _run_case(c)
    tied = (base[1][:, 1:] == base[1][:, :-1]).sum()
    assert int(tied) >= B, "the case must put tied pairs into the top K"
    for s in (0, 1, 2, 7, 0):
        old = ops.topk_splits(s)
        try:
            assert ops.topk_splits(-1) == s
            got = _run_case(c)
        finally:
            assert ops.topk_splits(old) == s
        for a, b in zip(got, base):
            assert torch.equal(a, b), f"splits={s}"
        assert torch.equal(got[1].view(torch.int32), base[1].view(torch.int32))


def test_graph_capture():
    """E = 128 with exclude and target: one capture, two replays with new
    queries, each equal to an eager call."""
    g = torch.Generator().manual_seed(2)
    B, E, V, K = 33, 128, 4099, 10
    q = torch.randn(B, E, generator=g).to(DEV)
    W = torch.randn(V, E, generator=g).to(DEV)
    bias = torch.randn(V, generator=g).to(DEV)
    excl = torch.randint(-1, V, (B, 5), generator=g).to(DEV)
    target = torch.randint(0, V, (B,), generator=g).to(DEV)
    ids = torch.empty(B, K, dtype=torch.int64, device=DEV)
    scores = torch.empty(B, K, device=DEV)
    rank = torch.empty(B, dtype=torch.int64, device=DEV)

    def call():
        ops.topk_scores(q, W, bias, K, ids, scores, 1, V - 1, exclude=excl, target=target,
                        out_rank=rank)

    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        call()
    torch.cuda.current_stream().wait_stream(s)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        call()
    for i in range(2):
        q.copy_(torch.randn(B, E, generator=g))
        graph.replay()
        torch.cuda.synchronize()
        got = (ids.clone(), scores.clone(), rank.clone())
        want = run_topk(q, W, bias, K, 1, V - 1, excl, target)
        torch.cuda.synchronize()
        for a, b in zip(got, want):
            assert torch.equal(a, b), f"replay {i}"


@pytest.mark.parametrize("E,heads", [(128, 2), (256, 4)])
def test_bert4rec_trainer_matches_cpu(E, heads):
    """recommend / eval_batch_full on the GPU against the CPU trainer with the
    same weights; the output layer holds integers, so score gaps are far above
    the fp32 differences of the two encoders."""
    kw = dict(n_items=30, max_len=6, embed_dim=E, n_heads=heads, n_layers=1, batch_size=4,
              dropout=0.0, seed=3)
    gpu = Bert4RecTrainer(device=DEV, **kw)
    cpu = Bert4RecTrainer(device="cpu", **kw)
    g = torch.Generator().manual_seed(0)
    with torch.no_grad():
        gpu.model.out.weight.copy_(torch.randint(-3, 4, (32, E), generator=g).float())
        gpu.model.out.bias.copy_(torch.randint(-2, 3, (32,), generator=g).float())
    cpu.item.store.weight.copy_(gpu.item.store.weight.cpu())
    cpu.opt.flat.copy_(gpu.opt.flat.cpu())
    with torch.no_grad():
        cpu.model.out.weight.copy_(gpu.model.out.weight.cpu())
        cpu.model.out.bias.copy_(gpu.model.out.bias.cpu())
    assert torch.equal(cpu.model.out.weight.detach(), gpu.model.out.weight.detach().cpu())
    seqs = torch.randint(1, 31, (4, 6), generator=g)
    seqs[0, :2] = 0
    seqs[:, -1] = 31
    for seen in (True, False):
        gi, gs = gpu.recommend(seqs.to(DEV), 10, exclude_seen=seen)
        ci, cs = cpu.recommend(seqs, 10, exclude_seen=seen)
        assert torch.equal(gi.cpu(), ci)
        torch.testing.assert_close(gs.cpu(), cs, rtol=1e-4, atol=1e-4)
    # Random targets: the ranks are equal. The metric sums are fp32 terms
    # 1 / log2(rank + 2) added by torch on either device, and a device's log2
    # and order of summation may round another way: with these targets at
    # hidden 256 the ranks were equal and NDCG@50 was 0.24488049745559692 on
    # the GPU, 0.24488048255443573 on the CPU (one fp32 ulp).
    targets = torch.randint(1, 31, (4,), generator=g)
    gr = gpu.eval_batch_full(seqs.to(DEV), targets.to(DEV))
    cr = cpu.eval_batch_full(seqs, targets)
    assert torch.equal(gr.cpu(), cr)
    gpu.pop_metrics_full()                                   # (clears the sums)
    cpu.pop_metrics_full()
    # So the metrics are compared on targets whose terms are exact: the items
    # the CPU trainer puts at positions 0, 2, 14 and 2 of all 30 (ranks 0, 2,
    # 14, 2 without ties; log2(rank + 2) = 1, 2, 4, 2). Every term is a power
    # of two and every partial sum exact in any order, so equal ranks must
    # give equal metrics bit for bit.
    order, _ = cpu.recommend(seqs, 30, exclude_seen=False)
    targets = order[torch.arange(4), torch.tensor([0, 2, 14, 2])]
    gr = gpu.eval_batch_full(seqs.to(DEV), targets.to(DEV))
    cr = cpu.eval_batch_full(seqs, targets)
    assert torch.equal(gr.cpu(), cr)
    assert gpu.pop_metrics_full() == cpu.pop_metrics_full()


def test_bert4rec_eval_batch_full_captures():
    """eval_batch_full at hidden 128 inside torch.cuda.graph: the replayed
    ranks equal the eager ones."""
    tr = Bert4RecTrainer(n_items=300, max_len=20, embed_dim=128, n_heads=2, n_layers=1,
                         batch_size=8, device=DEV, dropout=0.0, seed=4)
    g = torch.Generator().manual_seed(1)
    seqs = torch.randint(1, 301, (8, 20), generator=g)
    seqs[:, -1] = 301
    seqs = seqs.to(DEV)
    targets = torch.randint(1, 301, (8,), generator=g).to(DEV)
    want = tr.eval_batch_full(seqs, targets).clone()
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        tr.eval_batch_full(seqs, targets)
    torch.cuda.current_stream().wait_stream(s)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        rank = tr.eval_batch_full(seqs, targets)
    graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(rank, want)


@pytest.mark.parametrize("E", [96, 512])
def test_other_widths_are_refused(E):
    q = torch.zeros(2, E, device=DEV)
    W = torch.zeros(10, E, device=DEV)
    ids = torch.empty(2, 3, dtype=torch.int64, device=DEV)
    sc = torch.empty(2, 3, device=DEV)
    with pytest.raises(RuntimeError, match=r"topk_scores.*16, 32, 64, 128, 256"):
        ops.topk_scores(q, W, None, 3, ids, sc)
