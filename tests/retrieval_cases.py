"""Inputs shared by the retrieval tests (CPU and GPU): exact integer-valued
cases with heavy ties, and a brute-force full sort."""
import functools

import torch

from tdfo_amd import ops


def inner_range(V):
    """[1, V - 1): Bert4Rec's eligible ids (PAD = 0 and MASK = V - 1 dropped),
    empty where V is too small to hold one."""
    lo = min(1, V)
    return lo, max(lo, V - 1)


def run_topk(q, W, bias, k, v_lo, v_hi, exclude=None, target=None):
    """ops.topk_scores on the tensors' device -> (ids, scores, rank or None)."""
    B = q.shape[0]
    ids = torch.empty(B, k, dtype=torch.int64, device=q.device)
    scores = torch.empty(B, k, dtype=torch.float32, device=q.device)
    rank = torch.empty(B, dtype=torch.int64, device=q.device) if target is not None else None
    ops.topk_scores(q, W, bias, k, ids, scores, v_lo, v_hi, exclude=exclude, target=target,
                    out_rank=rank)
    return ids, scores, rank


def brute_force(q, W, bias, k, v_lo, v_hi, exclude=None, target=None):
    """Full sort of every row's eligible items by (-score, id) in fp64."""
    B, V = q.shape[0], W.shape[0]
    s = q.double() @ W.double().t()
    if bias is not None:
        s = s + bias.double()
    ids = torch.full((B, k), -1, dtype=torch.int64)
    scores = torch.full((B, k), float("-inf"), dtype=torch.float32)
    rank = torch.zeros(B, dtype=torch.int64)
    for b in range(B):
        banned = set() if exclude is None else {int(x) for x in exclude[b] if x >= 0}
        elig = [v for v in range(v_lo, v_hi) if v not in banned]
        elig.sort(key=lambda v: (-float(s[b, v]), v))
        for j, v in enumerate(elig[:k]):
            ids[b, j] = v
            scores[b, j] = float(s[b, v])
        if target is not None:
            t = int(target[b])
            rank[b] = sum(1 for v in elig if v != t and s[b, v] >= s[b, t])
    return ids, scores, (rank if target is not None else None)


@functools.lru_cache(maxsize=None)
def exact_case(E, B, V, K, X, full_range=False, seed=0):
    """CPU inputs whose every product and sum is exact in fp32, and the CPU
    reference's result on them (computed once per case, never modified).
    Few distinct W rows -> long runs of tied scores. Per row b the exclude
    list: b % 4 == 0 the top-1 repeated, 1 the head of the top-K (all of it
    when X >= K), 2 a duplicated head, 3 random ids including ineligible ones;
    -1 padding in all. Targets: b % 3 == 0 a top item (tied with its copies,
    possibly excluded), 1 a random id, 2 an id outside [v_lo, v_hi)."""
    g = torch.Generator().manual_seed(1000 * seed + E + 7 * B + 13 * K + X + V % 1009)
    ngroups = max(1, min(V, 37))
    base = torch.randint(-3, 4, (ngroups, E), generator=g).float()
    grp = torch.randint(0, ngroups, (V,), generator=g)
    W = base[grp].contiguous()
    bgrp = torch.randint(-2, 3, (ngroups,), generator=g).float()
    bias = bgrp[grp].clone()
    odd = torch.rand(V, generator=g) < 0.1
    bias[odd] = torch.randint(-2, 3, (int(odd.sum()),), generator=g).float()
    q = torch.randint(-3, 4, (B, E), generator=g).float()
    v_lo, v_hi = (0, V) if full_range else inner_range(V)
    top, _, _ = run_topk(q, W, bias, K, v_lo, v_hi)
    exclude = None
    if X > 0:
        exclude = torch.full((B, X), -1, dtype=torch.int64)
        for b in range(B):
            m = b % 4
            if m == 0:
                exclude[b, : max(1, X // 2)] = top[b, 0]
            elif m == 1:
                n = min(X, K)
                exclude[b, :n] = top[b, :n]
            elif m == 2:
                n = max(1, min(X // 2, K))
                exclude[b, :n] = top[b, :n]
                exclude[b, n: 2 * n] = top[b, :n][: X - n]
            else:
                r = torch.randint(0, V, (X,), generator=g)
                r[::5] = -1
                r[1::7] = 0
                r[2::7] = V - 1
                exclude[b] = r
    target = torch.randint(0, V, (B,), generator=g)
    for b in range(0, B, 3):
        t = int(top[b, min(K - 1, 3)])
        target[b] = t if t >= 0 else 0
    for b in range(2, B, 3):
        target[b] = 0 if b % 2 else V - 1
    ids, scores, rank = run_topk(q, W, bias, K, v_lo, v_hi, exclude, target)
    return dict(q=q, W=W, bias=bias, K=K, v_lo=v_lo, v_hi=v_hi, exclude=exclude, target=target,
                ids=ids, scores=scores, rank=rank)
