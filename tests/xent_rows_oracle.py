"""float64 oracle of the candidate-subset Linear + label-smoothed CE
(``ops.linear_xent_rows``: sampled softmax) and the shared cases of its tests.

Written out by hand (no autograd), independent of
``ops.reference.linear_xent_rows``; it materialises the [N, Mv] logits, so
shapes stay small. C = the non-hole candidates, Mv = |C|, nv = non-ignored
tokens:
    z[n, c] = H[n] . W[cand[c]] + bias[cand[c]] + corr[c]            (c in C)
    loss_n  = logsumexp_C z - (1 - eps) z[n, target[n]] - eps mean_C z
    dz      = (softmax_C z - eps / Mv - (1 - eps) onehot(target)) / nv   (0 if ignored)
    dH = dz W[cand],  dW[cand[c]] = sum_n dz[n, c] H[n],  db[cand[c]] = sum_n dz[n, c]
    mean    = sum_n loss_n / max(1, nv)

The bound is that of tests/xent_oracle.py: the maths, the MFMA and the
accumulation are the same.
"""
import functools

import torch

from tests import xent_oracle as xo
from tests.xent_oracle import BOUND, EPS, rel_err  # noqa: F401  (shared with the tests)

WIDTHS = (16, 32, 64, 128, 256)
V = 5003
# (N, M): the own tile (64) and the streamed tiles (128 / 64 / 32 rows) at their edges
SHAPES = [(7, 1), (7, 7), (65, 64), (65, 65), (64, 127), (320, 129), (320, 513), (1030, 2049)]
NAMES = ("dH", "loss", "dW", "db", "mean")
# chosen numbers of valid tokens (the 64-token own tile at its edges), at NV_SHAPE
NV = (1, 63, 64, 65, 129)
NV_SHAPE = (200, 129)       # (N, M)
NV_TWICE = (97, 257)        # two calls bit-identical, at (NV_TWICE_N, 129)
NV_TWICE_N = 264


def valid_slots(cand: torch.Tensor, V: int) -> torch.Tensor:
    return torch.nonzero((cand >= 0) & (cand < V)).view(-1)


@functools.lru_cache(maxsize=None)
def make_case(N: int, M: int, E: int, V: int = V, hs: float = 1.0, with_corr: bool = False,
              nv=None):
    """CPU inputs (H, W, b, cand, target, corr). About 30 % of the candidate
    slots are holes (-1, V or V + 5), the first and the last slot among them
    (M >= 3); rows 0 and V - 1 are candidates; about 60 % of the tokens are
    ignored (-1, M, M + 3 or a slot that is a hole); several tokens share one
    positive. With ``nv`` exactly that many tokens are valid, spread evenly over
    the N, the first on the first and the last on the last valid candidate, a
    third of them on one shared positive. Cached: treat as read-only."""
    g = torch.Generator().manual_seed(7919 * E + 31 * N + M + V)
    H = torch.randn(N, E, generator=g) * hs
    W = torch.randn(V, E, generator=g) * 0.2
    b = torch.randn(V, generator=g) * 0.1
    cand = torch.randperm(V - 2, generator=g)[:M] + 1          # distinct, in [1, V - 2]
    if M >= 3:
        hole = torch.rand(M, generator=g) < 0.3
        hole[0] = hole[M - 1] = True
        hole[1] = False
        hole[M // 2] = False
        kinds = torch.tensor([-1, V, V + 5])[torch.randint(0, 3, (M,), generator=g)]
        cand = torch.where(hole, kinds, cand)
    ok = valid_slots(cand, V)
    cand[ok[0]] = 0
    if ok.numel() > 1:
        cand[ok[-1]] = V - 1
    target = ok[torch.randint(0, ok.numel(), (N,), generator=g)]
    target[: N // 3] = ok[ok.numel() // 2]                       # a shared positive
    ign = torch.rand(N, generator=g) < 0.6
    kinds = torch.tensor([-1, M, M + 3])[torch.randint(0, 3, (N,), generator=g)]
    target = torch.where(ign, kinds, target)
    if M >= 3:
        target[1] = 0                                            # names a hole: ignored
    target[0], target[N - 1] = ok[0], ok[-1]
    if N > 4:
        target[2] = target[3] = ok[ok.numel() // 2]
    corr = torch.randn(M, generator=g) * 0.5 if with_corr else None
    if nv is not None:
        pos = xo.valid_positions(N, nv, "spread")
        lab = ok[torch.randint(0, ok.numel(), (nv,), generator=g)]
        lab[: nv // 3] = ok[ok.numel() // 2]
        if nv >= 1:
            lab[0] = ok[0]
        if nv >= 2:
            lab[nv - 1] = ok[-1]
        target = torch.tensor([-1, M, M + 3])[torch.randint(0, 3, (N,), generator=g)]
        target[pos] = lab
    return H, W, b, cand, target, corr


def oracle(H, W, b, cand, target, corr=None, eps=EPS):
    """-> (dH, lossv, dW [V, E], db [V], mean loss, db_terms [V]), float64;
    dW / db are zero outside the rows named by valid candidates. db_terms is
    the magnitude of the terms db sums (xent_oracle.db_err)."""
    H, W, b = H.double(), W.double(), b.double()
    N, V, M = H.shape[0], W.shape[0], cand.numel()
    slots = valid_slots(cand, V)
    rows = cand[slots]
    Mv = slots.numel()
    pos = torch.full((M,), -1, dtype=torch.int64)
    pos[slots] = torch.arange(Mv)
    inr = (target >= 0) & (target < M)
    y = torch.where(inr, pos[target.clamp(0, M - 1)], -torch.ones_like(target))      # (M >= 1)
    valid = y >= 0
    nv = max(1, int(valid.sum()))
    dW, db = torch.zeros_like(W), torch.zeros_like(b)
    if Mv == 0:
        zero = torch.zeros((), dtype=torch.float64)
        return torch.zeros_like(H), zero.expand(N).clone(), dW, db, zero, torch.zeros_like(b)
    z = H @ W[rows].t() + b[rows]
    if corr is not None:
        z = z + corr.double()[slots]
    lse = torch.logsumexp(z, 1)
    yc = y.clamp_min(0)
    zy = z.gather(1, yc.view(-1, 1)).view(-1)
    lossv = torch.where(valid, lse - (1 - eps) * zy - eps * z.mean(1), torch.zeros_like(lse))
    dz = torch.exp(z - lse[:, None]) - eps / Mv
    dz[torch.arange(N), yc] -= 1 - eps
    dz = dz * valid[:, None] / nv
    dW[rows] = dz.t() @ H
    db[rows] = dz.sum(0)
    terms = torch.zeros_like(b)
    terms[rows] = 2 * (torch.exp(z - lse[:, None]) * valid[:, None]).sum(0) / nv - db[rows]
    return dz @ W[rows], lossv, dW, db, lossv.sum() / nv, terms


@functools.lru_cache(maxsize=None)
def oracle_case(N: int, M: int, E: int, V: int = V, hs: float = 1.0, with_corr: bool = False,
                nv=None):
    """Cached: treat as read-only."""
    H, W, b, cand, target, corr = make_case(N, M, E, V, hs, with_corr, nv)
    return oracle(H, W, b, cand, target, corr)


def n_valid(cand, target, V: int) -> int:
    M = cand.numel()
    inr = (target >= 0) & (target < M)
    c = cand[target.clamp(0, M - 1)]
    return int((inr & (c >= 0) & (c < V)).sum())


def named_rows(cand, V: int) -> torch.Tensor:
    """bool [V]: the rows of dW / db a call assigns"""
    m = torch.zeros(V, dtype=torch.bool)
    m[cand[valid_slots(cand, V)]] = True
    return m


def on_named(out, named):
    """[dH, lossv, dW, db, mean] -> {name: tensor}, dW / db on the named rows"""
    d = dict(zip(NAMES, [out[0], out[1], out[2].cpu()[named], out[3].cpu()[named], out[4]]))
    if len(out) > 5:
        d["db_terms"] = out[5][named]
    return d


@functools.lru_cache(maxsize=None)
def ref_err(N: int, M: int, E: int, V: int = V, hs: float = 1.0, with_corr: bool = False,
            nv=None):
    """{name: row_err of ``ops.reference.linear_xent_rows`` in float32 on the
    CPU against the oracle}: the yardstick of the per-row bound, once per
    case. dW / db are compared on the named rows only."""
    from tdfo_amd.ops import reference as ref

    H, W, b, cand, target, corr = make_case(N, M, E, V, hs, with_corr, nv)
    out = [torch.zeros_like(H), torch.zeros(N), torch.zeros_like(W), torch.zeros_like(b)]
    k = ref.linear_xent_rows(H, W, b, cand, target, EPS, *out, corr=corr)
    assert k == n_valid(cand, target, V)
    named = named_rows(cand, V)
    want = oracle_case(N, M, E, V, hs, with_corr, nv)
    return xo.errs(on_named(out + [out[1].sum() / max(1, k)], named), on_named(want, named))


def assert_within(out, args, tag):
    """The kernel's [dH, lossv, dW, db, mean] on ``make_case(*args)`` within
    the per-row bound of tests/xent_oracle.py"""
    cand = make_case(*args)[3]
    Vv = args[3] if len(args) > 3 else V
    named = named_rows(cand, Vv)
    xo.assert_bound(xo.errs(on_named(out, named), on_named(oracle_case(*args), named)),
                    ref_err(*args), tag)


def without_holes(cand, target, V, corr=None):
    """The same problem with the holes removed and the targets remapped."""
    M = cand.numel()
    slots = valid_slots(cand, V)
    pos = torch.full((M,), -1, dtype=torch.int64)
    pos[slots] = torch.arange(slots.numel())
    inr = (target >= 0) & (target < M)
    t2 = torch.where(inr, pos[target.clamp(0, M - 1)], -torch.ones_like(target))
    return cand[slots].contiguous(), t2, (None if corr is None else corr[slots].contiguous())


def candidate_case(N: int = 1030, S: int = 512, n_items: int = 3000, seed: int = 3):
    """labels [N] (about a third ignored = 0) and negatives [S] with repeats
    among themselves and one negative equal to a label."""
    g = torch.Generator().manual_seed(seed)
    labels = torch.randint(1, n_items + 1, (N,), generator=g)
    labels[torch.rand(N, generator=g) < 0.35] = 0
    labels[5], labels[6] = 17, 17
    neg = torch.randint(1, n_items + 1, (S,), generator=g)
    neg[3] = neg[4] = neg[100]
    neg[7] = labels[5]
    return labels, neg


def check_candidates(labels, neg, cand, target, ignore=0):
    """The properties ops.xent_candidates promises."""
    labels, neg, cand, target = labels.cpu(), neg.cpu(), cand.cpu(), target.cpu()
    assert cand.numel() == labels.numel() + neg.numel() and target.numel() == labels.numel()
    live = cand[cand >= 0]
    want = torch.unique(torch.cat([labels[labels != ignore], neg]))
    assert live.numel() == torch.unique(live).numel(), "valid candidates repeat"
    assert torch.equal(torch.sort(live).values, want), "valid candidates are not the union"
    assert bool((cand[cand < 0] == -1).all())
    on = labels != ignore
    assert bool((target[~on] == -1).all())
    assert bool((target[on] >= 0).all()) and bool((target[on] < cand.numel()).all())
    assert torch.equal(cand[target[on]], labels[on])
