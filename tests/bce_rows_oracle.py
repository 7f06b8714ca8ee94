"""float64 oracle of the shared-negative Linear + BCE / gBCE
(``ops.linear_bce_rows``) and the shared cases of its tests.

Written out by hand (no autograd), independent of
``ops.reference.linear_bce_rows``; it materialises the [N, Sv] logits, so
shapes stay small. Cn = the non-hole negatives, Sv = |Cn|, nv = non-ignored
tokens, y = labels[n]:
    z[n, c] = H[n] . W[negs[c]] + bias[negs[c]]                     (c in Cn)
    zy[n]   = H[n] . W[y] + bias[y]
    K[n]    = Sv - [y in Cn]
    loss_n  = (beta softplus(-zy) + sum_{c: negs[c] != y} softplus(z[n, c])) / (K[n] + 1)
    dz      = sigmoid(z) / ((K + 1) nv)       (0 where negs[c] == y, 0 if ignored)
    dzy     = -beta sigmoid(-zy) / ((K + 1) nv)
    dH = dz W[negs] + dzy W[y],  dW[negs[c]] = sum_n dz[n, c] H[n],  dW[y] += dzy[n] H[n]
    mean    = sum_n loss_n / max(1, nv)

The bound is that of tests/xent_oracle.py: products, MFMA and accumulation
lengths are those of the kernels it already covers; an fp32 evaluation of
these formulas at every shape below stays within 1e-6 of fp64 under rel_err,
and no output's magnitude vanishes.
"""
import functools

import torch

from tests import xent_oracle as xo
from tests.xent_oracle import BOUND, rel_err  # noqa: F401  (shared with the tests)

WIDTHS = (16, 32, 64, 128, 256)
V = 5003
IGNORE = 0
BETAS = (1.0, 0.3)
# (N, S): the own tile (64) and the streamed tiles (128 / 64 / 32 rows) at their edges
SHAPES = [(7, 1), (7, 7), (65, 64), (65, 65), (64, 127), (320, 129), (320, 513), (1030, 2049)]
# (N, S, V, hs): the shapes above, one with saturating scores, one at a larger V
CASES = [(N, S, V, 1.0) for N, S in SHAPES] + [(320, 513, V, 12.0), (65, 65, 70001, 1.0)]
NAMES = ("dH", "loss", "dW", "db", "mean")
# chosen numbers of valid tokens, and lengths of the hot label's run (one wave
# walks a run 64 tokens at a time), at NV_SHAPE
NV = (1, 63, 64, 65, 129)
HOT = (63, 64, 65)
HOT_NV = 129
NV_SHAPE = (200, 129)       # (N, S)
NV_TWICE = (97, 257)        # two calls bit-identical, at (NV_TWICE_N, 129)
NV_TWICE_N = 264


def valid_negs(negs: torch.Tensor, V: int) -> torch.Tensor:
    return negs[(negs >= 0) & (negs < V)]


def valid_tokens(labels: torch.Tensor, V: int, ignore: int = IGNORE) -> torch.Tensor:
    return (labels != ignore) & (labels >= 0) & (labels < V)


def label_order(labels: torch.Tensor, V: int, ignore: int = IGNORE) -> torch.Tensor:
    """int32 token indices stably sorted by label, ignored tokens last."""
    key = torch.where(valid_tokens(labels, V, ignore), labels, torch.full_like(labels, 2 ** 40))
    return torch.sort(key, stable=True).indices.to(torch.int32)


@functools.lru_cache(maxsize=None)
def make_case(N: int, S: int, E: int, V: int = V, hs: float = 1.0, nv=None, hot=None):
    """CPU inputs (H, W, b, labels, order, negs). The valid negatives are
    distinct and ascending, rows 0 and V - 1 among them (S >= 2); about 30 % of
    the slots are holes (-1, V or V + 5), the first and the last slot among them
    (S >= 3). The first third of the tokens shares one label that is no
    negative (a quarter of them ignored); of the others about three quarters
    are ignored (0, -3, V or V + 7), which makes about 60 % in all, and a quarter
    of the rest have a label that is one of the negatives. With ``nv`` exactly
    that many tokens are valid, spread evenly over the N; ``hot`` of them (a
    third by default) share the one label that is no negative, the last two
    share a label that is a negative. Cached: treat as read-only."""
    g = torch.Generator().manual_seed(7919 * E + 31 * N + S + V)
    H = torch.randn(N, E, generator=g) * hs
    W = torch.randn(V, E, generator=g) * 0.2
    b = torch.randn(V, generator=g) * 0.1
    perm = torch.randperm(V - 2, generator=g) + 1              # distinct, in [1, V - 2]
    negs = torch.sort(perm[:S]).values
    spare = perm[S:]                                           # rows that are no negative
    if S >= 3:
        hole = torch.rand(S, generator=g) < 0.3
        hole[0] = hole[S - 1] = True
        hole[1] = False
        hole[S // 2] = False
        kinds = torch.tensor([-1, V, V + 5])[torch.randint(0, 3, (S,), generator=g)]
        negs = torch.where(hole, kinds, negs)
    ok = torch.nonzero((negs >= 0) & (negs < V)).view(-1)
    negs[ok[0]] = 0
    if ok.numel() > 1:
        negs[ok[-1]] = V - 1
    rows = negs[ok]
    hits = rows[rows != IGNORE]                                # (a label 0 would be ignored)
    labels = spare[torch.randint(0, spare.numel(), (N,), generator=g)]       # the assign path
    if hits.numel():
        hit = torch.rand(N, generator=g) < 0.25
        labels = torch.where(hit, hits[torch.randint(0, hits.numel(), (N,), generator=g)], labels)
    third = N // 3
    labels[:third] = spare[0]                                  # one long run
    ign = torch.rand(N, generator=g) < torch.where(torch.arange(N) < third, 0.25, 0.78)
    kinds = torch.tensor([IGNORE, -3, V, V + 7])[torch.randint(0, 4, (N,), generator=g)]
    labels = torch.where(ign, kinds, labels)
    labels[0] = spare[0]
    labels[N - 1] = hits[-1] if hits.numel() else spare[1]
    if N > 4:
        labels[N - 2] = labels[N - 1]                          # a short run on the add path
    if N >= 320 and nv is None:
        assert int((labels == spare[0]).sum()) > 64
    if nv is not None:
        pos = xo.valid_positions(N, nv, "spread")
        lab = spare[1 + torch.randint(0, spare.numel() - 1, (nv,), generator=g)]
        if hits.numel():
            hit = torch.rand(nv, generator=g) < 0.25
            lab = torch.where(hit, hits[torch.randint(0, hits.numel(), (nv,), generator=g)], lab)
        run = nv // 3 if hot is None else hot
        assert run <= nv
        lab[:run] = spare[0]
        if nv - run >= 2:
            lab[nv - 2:] = hits[-1] if hits.numel() else spare[1]
        labels = torch.tensor([IGNORE, -3, V, V + 7])[torch.randint(0, 4, (N,), generator=g)]
        labels[pos] = lab
        assert int((labels == spare[0]).sum()) == run
    return H, W, b, labels, label_order(labels, V), negs


def _softplus(z):
    return z.clamp_min(0) + torch.log1p(torch.exp(-z.abs()))


def _sigmoid(z):
    e = torch.exp(-z.abs())
    return torch.where(z >= 0, torch.ones_like(e), e) / (1 + e)


def oracle(H, W, b, labels, negs, beta=1.0, ignore=IGNORE):
    """-> (dH, lossv, dW [V, E], db [V], mean loss, db_terms [V]), float64;
    dW / db are zero outside the rows named by valid negatives and valid
    labels. db_terms is the magnitude of the terms db sums: a row that is a
    negative and a label sums terms of both signs (xent_oracle.db_err)."""
    H, W, b = H.double(), W.double(), b.double()
    V = W.shape[0]
    rows = valid_negs(negs, V)
    valid = valid_tokens(labels, V, ignore)
    nv = max(1, int(valid.sum()))
    y = torch.where(valid, labels, torch.zeros_like(labels))
    z = H @ W[rows].t() + b[rows]
    zy = (H * W[y]).sum(1) + b[y]
    keep = (rows.view(1, -1) != y.view(-1, 1)).double()
    k1 = keep.sum(1) + 1
    vd = valid.double()
    lossv = (beta * _softplus(-zy) + (_softplus(z) * keep).sum(1)) / k1 * vd
    dz = _sigmoid(z) * keep * (vd / (k1 * nv))[:, None]
    dzy = -beta * _sigmoid(-zy) * vd / (k1 * nv)
    dW, db = torch.zeros_like(W), torch.zeros_like(b)
    dW[rows] = dz.t() @ H
    db[rows] = dz.sum(0)
    dW.index_add_(0, y, dzy[:, None] * H)
    db.index_add_(0, y, dzy)
    terms = torch.zeros_like(b)
    terms[rows] = dz.sum(0)
    terms.index_add_(0, y, -dzy)
    return dz @ W[rows] + dzy[:, None] * W[y], lossv, dW, db, lossv.sum() / nv, terms


@functools.lru_cache(maxsize=None)
def oracle_case(N: int, S: int, E: int, V: int = V, hs: float = 1.0, beta: float = 1.0,
                nv=None, hot=None):
    """Cached: treat as read-only."""
    H, W, b, labels, _, negs = make_case(N, S, E, V, hs, nv, hot)
    return oracle(H, W, b, labels, negs, beta)


def named_rows(labels, negs, V, ignore=IGNORE) -> torch.Tensor:
    """bool [V]: the rows of dW / db a call assigns (none without a valid token)."""
    m = torch.zeros(V, dtype=torch.bool)
    valid = valid_tokens(labels, V, ignore)
    if bool(valid.any()):
        m[valid_negs(negs, V)] = True
        m[labels[valid]] = True
    return m


def on_named(out, named):
    """[dH, lossv, dW, db, mean] -> {name: tensor}, dW / db on the named rows"""
    d = dict(zip(NAMES, [out[0], out[1], out[2].cpu()[named], out[3].cpu()[named], out[4]]))
    if len(out) > 5:
        d["db_terms"] = out[5][named]
    return d


@functools.lru_cache(maxsize=None)
def ref_err(N: int, S: int, E: int, V: int = V, hs: float = 1.0, beta: float = 1.0, nv=None,
            hot=None):
    """{name: row_err of ``ops.reference.linear_bce_rows`` in float32 on the
    CPU against the oracle}: the yardstick of the per-row bound, once per
    case. dW / db are compared on the named rows only."""
    from tdfo_amd.ops import reference as ref

    H, W, b, labels, _, negs = make_case(N, S, E, V, hs, nv, hot)
    out = [torch.zeros_like(H), torch.zeros(N), torch.zeros_like(W), torch.zeros_like(b)]
    k = ref.linear_bce_rows(H, W, b, labels, negs, beta, IGNORE, *out)
    assert k == int(valid_tokens(labels, V).sum())
    named = named_rows(labels, negs, V)
    want = oracle_case(N, S, E, V, hs, beta, nv, hot)
    return xo.errs(on_named(out + [out[1].sum() / max(1, k)], named), on_named(want, named))


def assert_within(out, args, tag):
    """The kernel's [dH, lossv, dW, db, mean] on the case ``args`` = (N, S, E,
    V, hs, beta, nv, hot) within the per-row bound of tests/xent_oracle.py"""
    N, S, E, Vv, hs, beta, nv, hot = args
    _, _, _, labels, _, negs = make_case(N, S, E, Vv, hs, nv, hot)
    named = named_rows(labels, negs, Vv)
    xo.assert_bound(xo.errs(on_named(out, named), on_named(oracle_case(*args), named)),
                    ref_err(*args), tag)


def candidate_case(N: int = 1030, S: int = 512, n_items: int = 3000, seed: int = 3):
    """labels [N] (about a third ignored = 0) with repeated labels, and
    negatives [S] with repeats among themselves and one equal to a label."""
    g = torch.Generator().manual_seed(seed)
    labels = torch.randint(1, n_items + 1, (N,), generator=g)
    labels[torch.rand(N, generator=g) < 0.35] = 0
    labels[5], labels[6], labels[900] = 17, 17, 17
    neg = torch.randint(1, n_items + 1, (S,), generator=g)
    neg[3] = neg[4] = neg[100]
    neg[7] = labels[5]
    return labels, neg


def check_candidates(labels, neg, negs, order, V, ignore=IGNORE):
    """The properties ops.bce_candidates promises."""
    labels, neg, negs, order = labels.cpu(), neg.cpu(), negs.cpu(), order.cpu()
    assert negs.numel() == neg.numel() and order.numel() == labels.numel()
    assert order.dtype == torch.int32
    live = negs[negs >= 0]
    assert bool((negs[negs < 0] == -1).all())
    assert bool((live[1:] > live[:-1]).all()), "valid negatives are not distinct and ascending"
    assert torch.equal(live, torch.unique(neg[(neg >= 0) & (neg < V)])), "not the unique negatives"
    o = order.long()
    assert torch.equal(torch.sort(o).values, torch.arange(labels.numel())), "not a permutation"
    lab = labels[o]
    on = valid_tokens(lab, V, ignore)
    nv = int(on.sum())
    assert bool(on[:nv].all()), "ignored tokens are not last"
    # equal labels adjacent (sorted), token indices ascending inside a run
    lab, o = lab[:nv], o[:nv]
    same = lab[1:] == lab[:-1]
    assert bool((lab[1:] >= lab[:-1]).all())
    assert bool((o[1:][same] > o[:-1][same]).all())
