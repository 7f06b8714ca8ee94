"""Float64 oracles, per-element error bounds and shared inputs for the sparse
kernels (embedding bag forward, fused embedding backward + optimizer, pairwise
interaction), used by the CPU self-check (test_sparse_oracle.py) and by the
GPU width tests (test_gpu_sparse_widths.py).

The oracles are plain float64 torch on CPU tensors: no kernels and nothing
from ``tdfo_amd.ops.reference`` beyond the optimizer codes. Every input is
built once on the CPU from a seeded generator and cached; callers move copies
to their device and never write to a cached tensor. The ``run_*`` helpers at
the end call ``ops.*`` on a chosen device (CPU: the fp32 references, GPU: the
HIP kernels) and the ``check_*`` helpers hold the assertions both share.

Bounds (u23 = 2^-23, u8 = 2^-8, none measured on the code under test):
  embedding forward   |got - exact| <= (len + 2) u23 sum|psw W|  (+ u8 |exact|
                      for one round-to-nearest-even into bf16)
  embedding backward  the project's: max|got - exact| < 1e-4 max(1, max|exact|)
                      for W and dense_grad, 1e-3 for optimizer states
  interaction         |got - exact| <= u8 |exact| + (n + 2) u23 sum|terms|,
                      n = D forward, F backward, F + 1 for the dense slot:
                      twice the IEEE sequential bound, because the MFMA's
                      internal accumulation order and rounding are not
                      documented. A bound of 0 means exactly 0.
"""
import functools

import torch

from tdfo_amd.ops.reference import (EMB_ADAGRAD, EMB_ADAM, EMB_DENSE_GRAD, EMB_ROWWISE_ADAGRAD,
                                    EMB_SGD)

WIDTHS = (16, 32, 64, 128, 256, 512)
ALL_OPTS = (EMB_SGD, EMB_ROWWISE_ADAGRAD, EMB_ADAM, EMB_ADAGRAD, EMB_DENSE_GRAD)
U23 = 2.0 ** -23
U8 = 2.0 ** -8
SENTINEL = 7.0

EPS, BETA1, BETA2 = 1e-8, 0.9, 0.999
WEIGHT_DECAY = 0.01
HYPER = (0.05, 3.0)


def _gen(*seed):
    s = 0
    for v in seed:
        s = s * 1000003 + int(v) + 1
    return torch.Generator().manual_seed(s % (2 ** 31))


def _row_offset(rows):
    ro = torch.zeros(len(rows), dtype=torch.int64)
    ro[1:] = torch.tensor(rows[:-1], dtype=torch.int64).cumsum(0)
    return ro


def _bags(lens, rows, B, g):
    """indices / offsets of T * B bags (table-major) with the given lengths."""
    offs = torch.zeros(lens.numel() + 1, dtype=torch.int64)
    offs[1:] = lens.cumsum(0)
    tab = torch.repeat_interleave(torch.arange(lens.numel()) // B, lens)
    hi = torch.tensor(rows, dtype=torch.int64)[tab]
    idx = (torch.rand(tab.numel(), generator=g, dtype=torch.float64) * hi).long().clamp_max(hi - 1)
    return idx, offs


# ------------------------------------------------------- embedding forward
def embedding_bag_fwd(W, row_offset, indices, offsets, out_off, T, B, out_stride, psw=None,
                      mean=False):
    """-> (exact, mag, lens, written), each [B, out_stride]: the pooled rows at
    out[b, out_off[t] : out_off[t] + D] in float64, sum|psw W| of the same
    terms (divided by the bag length with ``mean``), the bag length behind
    every element, and which elements the op writes."""
    D = W.shape[1]
    ln = offsets[1:] - offsets[:-1]
    bag = torch.repeat_interleave(torch.arange(T * B), ln)
    vals = W[row_offset[bag // B] + indices].double()
    if psw is not None:
        vals = vals * psw.double()[:, None]
    pooled = torch.zeros(T * B, D, dtype=torch.float64).index_add_(0, bag, vals)
    mag = torch.zeros(T * B, D, dtype=torch.float64).index_add_(0, bag, vals.abs())
    if mean:
        div = ln.clamp_min(1).double()[:, None]
        pooled, mag = pooled / div, mag / div
    exact = torch.zeros(B, out_stride, dtype=torch.float64)
    emag = torch.zeros(B, out_stride, dtype=torch.float64)
    elen = torch.zeros(B, out_stride, dtype=torch.float64)
    written = torch.zeros(B, out_stride, dtype=torch.bool)
    for t in range(T):
        c = slice(int(out_off[t]), int(out_off[t]) + D)
        exact[:, c] = pooled[t * B:(t + 1) * B]
        emag[:, c] = mag[t * B:(t + 1) * B]
        elen[:, c] = ln[t * B:(t + 1) * B].double()[:, None]
        written[:, c] = True
    return exact, emag, elen, written


def fwd_bound(exact, mag, lens, bf16_out):
    b = (lens + 2.0) * U23 * mag
    return b + U8 * exact.abs() if bf16_out else b


def check_fwd(out, oracle, sentinel=SENTINEL):
    """Every written element within its bound (no exemptions), every other
    element still the sentinel; compared on the oracle's device. Returns the
    worst error / bound ratio."""
    exact, mag, lens, written = oracle
    got = out.detach().to(exact.device).double().view(exact.shape)
    bound = fwd_bound(exact, mag, lens, out.dtype == torch.bfloat16)
    err = (got - exact).abs()
    bad = written & ~(err <= bound)
    assert not bool(bad.any()), (int(bad.sum()), float(err[bad].max()))
    assert bool((got[~written] == sentinel).all()), "an element outside every slot was written"
    nz = written & (bound > 0)
    return float((err[nz] / bound[nz]).max()) if bool(nz.any()) else 0.0


FWD_LENS = (0, 1, 2, 5, 63, 64, 65, 130)
FWD_MODES = (("bf16", False, False), ("fp32", True, False), ("bf16", True, True),
             ("fp32", False, True))          # (out dtype, psw, mean)


@functools.lru_cache(maxsize=None)
def fwd_multihot_case(D):
    """T = 3, B = 70 (no multiple of any bags-per-wave), rows [100, 7, 1] (the
    one-row table: every id of a bag hits one row), bag lengths drawn per bag
    from FWD_LENS (lane groups of a wave run different trip counts, up to 3
    staging chunks), output slots permuted, 8 pad columns per row."""
    T, B, rows = 3, 70, [100, 7, 1]
    g = _gen(1, D)
    lens = torch.tensor(FWD_LENS)[torch.randint(0, len(FWD_LENS), (T * B,), generator=g)]
    idx, offs = _bags(lens, rows, B, g)
    return dict(T=T, B=B, D=D, W=torch.randn(sum(rows), D, generator=g), ro=_row_offset(rows),
                idx=idx, offs=offs, psw=torch.rand(idx.numel(), generator=g) + 0.5,
                out_off=torch.tensor([2 * D, 0, D], dtype=torch.int64), out_stride=T * D + 8)


def fwd_onehot_bpw(D):
    """Bags per wave of emb_fwd_onehot_kernel: 64 / min(D / 4, 64) lanes per bag."""
    return 64 // min(D // 4, 64)


def fwd_onehot_large_bags(D):
    """One more than fills the one-hot forward's grid once: the grid is capped
    at 8192 blocks of 4 waves of BPW bags, and a lane group takes a second bag
    in flight (``has1``) only past 8192 * 4 * BPW bags."""
    return 8192 * 4 * fwd_onehot_bpw(D) + 37


@functools.lru_cache(maxsize=2)
def fwd_onehot_case(D, large):
    if large:
        T, B, rows = 1, fwd_onehot_large_bags(D), [5000]
    else:
        T, B, rows = 5, 3001, [100, 7, 5000, 1, 70000]
    g = _gen(2, D, large)
    idx, offs = _bags(torch.ones(T * B, dtype=torch.int64), rows, B, g)
    return dict(T=T, B=B, D=D, W=torch.randn(sum(rows), D, generator=g), ro=_row_offset(rows),
                idx=idx, offs=offs, psw=torch.rand(T * B, generator=g) + 0.5,
                out_off=torch.arange(T, dtype=torch.int64) * D, out_stride=T * D + 8)


def fwd_onehot_oracle(c, use_psw, dev="cpu"):
    """One id per bag: the exact output is W[row] * psw. Computed in float64 on
    ``dev`` (the large case has half a million bags)."""
    T, B, D = c["T"], c["B"], c["D"]
    W, idx, ro = c["W"].to(dev), c["idx"].to(dev), c["ro"].to(dev)
    rows = ro[torch.arange(T * B, device=dev) // B] + idx
    vals = W[rows].double()
    if use_psw:
        vals = vals * c["psw"].to(dev).double()[:, None]
    exact = torch.zeros(B, c["out_stride"], dtype=torch.float64, device=dev)
    exact[:, :T * D] = vals.view(T, B, D).transpose(0, 1).reshape(B, T * D)
    written = torch.zeros_like(exact, dtype=torch.bool)
    written[:, :T * D] = True
    return exact, exact.abs(), torch.ones_like(exact), written


# ------------------------------------------- embedding backward + optimizer
def embedding_grad_rows(D, row_offset, indices, offsets, grad_off, T, B, grad, grad_stride,
                        psw=None, mean=False):
    """-> (rows [U] sorted unique global rows, g [U, D] float64 summed
    gradients). ``grad`` is fp32 or bf16 (upcast exactly)."""
    ln = offsets[1:] - offsets[:-1]
    bag = torch.repeat_interleave(torch.arange(T * B), ln)
    t = bag // B
    b = bag - t * B
    base = b * grad_stride + grad_off[t]
    g = grad.reshape(-1)[(base[:, None] + torch.arange(D)[None, :]).reshape(-1)]
    g = g.double().view(-1, D)
    scale = torch.ones(bag.numel(), dtype=torch.float64)
    if psw is not None:
        scale = scale * psw.double()
    if mean:
        scale = scale / ln[bag].double()
    uniq, inv = torch.unique(row_offset[t] + indices, return_inverse=True)
    acc = torch.zeros(uniq.numel(), D, dtype=torch.float64).index_add_(0, inv, g * scale[:, None])
    return uniq, acc


def embedding_opt(W, rows, g, opt, hyper, state1=None, state2=None, dense_grad=None, eps=EPS,
                  beta1=BETA1, beta2=BETA2, weight_decay=0.0):
    """One optimizer step of the touched ``rows`` from their summed gradients
    ``g``, in float64, with the formulas of the project's reference. Returns
    {"W", "s1", "s2", "dg"}: the new values of those rows only ([U, D]; [U]
    for the row-wise state), or None where the optimizer has no such tensor.
    hyper = [lr, step, (unscale), (skip)]; a skipped step returns None."""
    h = [float(x) for x in hyper.double().view(-1)]
    if len(h) > 3 and h[3] > 0:
        return None
    if len(h) > 2:
        g = g * h[2]
    lr = h[0]
    D = W.shape[1]
    w = W[rows].double()
    out = dict(W=None, s1=None, s2=None, dg=None)
    if opt == EMB_SGD:
        w = w - lr * (g + weight_decay * w)
    elif opt == EMB_ROWWISE_ADAGRAD:
        gg = g + weight_decay * w
        st = state1.view(-1)[rows].double() + (gg * gg).mean(1)
        out["s1"] = st
        w = w - (lr / (st.sqrt() + eps))[:, None] * gg
    elif opt == EMB_ADAGRAD:
        gg = g + weight_decay * w
        st = state1.view(-1, D)[rows].double() + gg * gg
        out["s1"] = st
        w = w - lr * gg / (st.sqrt() + eps)
    elif opt == EMB_ADAM:
        step = h[1]
        m = state1.view(-1, D)[rows].double() * beta1 + (1 - beta1) * g
        v = state2.view(-1, D)[rows].double() * beta2 + (1 - beta2) * g * g
        out["s1"], out["s2"] = m, v
        bc1 = 1 - beta1 ** step
        bc2 = 1 - beta2 ** step
        w = w - lr * ((m / bc1) / ((v / bc2).sqrt() + eps) + weight_decay * w)
    elif opt == EMB_DENSE_GRAD:
        out["dg"] = dense_grad.view(-1, D)[rows].double() + g
        return out
    else:
        raise ValueError(opt)
    out["W"] = w
    return out


def make_states(opt, nrows, D, g):
    """torch.rand optimizer states (and a random dense-gradient accumulator:
    the backward adds to it)."""
    s1 = s2 = dg = None
    if opt == EMB_ROWWISE_ADAGRAD:
        s1 = torch.rand(nrows, generator=g)
    elif opt in (EMB_ADAGRAD, EMB_ADAM):
        s1 = torch.rand(nrows * D, generator=g)
    if opt == EMB_ADAM:
        s2 = torch.rand(nrows * D, generator=g)
    if opt == EMB_DENSE_GRAD:
        dg = torch.randn(nrows * D, generator=g)
    return s1, s2, dg


def check_bwd(got, before, rows, exact, D):
    """got / before: {"W", "s1", "s2", "dg"} tensors after / before the step
    (any device). Touched rows within the project's tolerances of ``exact``
    (None: a skipped step, nothing may change); every other row bitwise
    unchanged. Returns the worst scaled errors {name: err / max(1, max|exact|)}."""
    tol = dict(W=1e-4, s1=1e-3, s2=1e-3, dg=1e-4)
    worst = {}
    for name in ("W", "s1", "s2", "dg"):
        a, b = got.get(name), before.get(name)
        if a is None:
            continue
        a, b = a.detach().cpu(), b.detach().cpu()
        cols = a.numel() // before["W"].shape[0]      # D, or 1 for the row-wise state
        a2, b2 = a.view(-1, cols), b.view(-1, cols)
        ex = None if exact is None else exact[name]
        if ex is None:
            assert torch.equal(a2, b2), f"{name} changed"
            continue
        untouched = torch.ones(a2.shape[0], dtype=torch.bool)
        untouched[rows] = False
        assert torch.equal(a2[untouched], b2[untouched]), f"{name}: an untouched row changed"
        ex = ex.view(rows.numel(), -1)
        err = float((a2[rows].double() - ex).abs().max())
        scale = max(1.0, float(ex.abs().max()))
        worst[name] = err / scale
        assert err < tol[name] * scale, (name, err, scale)
    return worst


BWD_ROWS = (3, 500, 40)
BWD_LENS = (0, 1, 2, 3, 7, 64, 65, 130)
# (name, B, one id per bag, bf16 grad, psw, mean)
BWD_PATHS = (("general-f32-sum", 250, False, False, False, False),
             ("general-bf16-psw-mean", 250, False, True, True, True),
             ("onehot256-f32", 256, True, False, False, False),
             ("onehot250-bf16", 250, True, True, False, False))


def _bwd_case(tag, D, T, B, rows, lens, bf16, use_psw, mean, gscale=1.0, tables=None):
    """``rows``: row count behind each of the T virtual tables; ``tables``:
    the physical tables when several virtual ones share rows (run-major)."""
    g = _gen(3, D, *[ord(ch) for ch in tag[:6]], B)
    idx, offs = _bags(lens, rows, B, g)
    stride = T * D + 8
    grad = torch.randn(B * stride, generator=g) * gscale
    if bf16:
        grad = grad.to(torch.bfloat16)
    goff = torch.tensor([((t + 1) % T) * D for t in range(T)], dtype=torch.int64)
    psw = (torch.rand(idx.numel(), generator=g) + 0.5) if use_psw else None
    tables = list(rows) if tables is None else list(tables)
    ro = _row_offset(tables).repeat(T // len(tables))
    c = dict(T=T, B=B, D=D, rows=tables, W=torch.randn(sum(tables), D, generator=g), ro=ro,
             idx=idx, offs=offs, goff=goff, grad=grad, stride=stride, psw=psw, mean=mean,
             hyper=torch.tensor(HYPER), seed=(3, D, B, len(tag)))
    c["urows"], c["g"] = embedding_grad_rows(D, ro, idx, offs, goff, T, B, grad, stride,
                                             psw=psw, mean=mean)
    return c


@functools.lru_cache(maxsize=4)
def bwd_case(D, path):
    """Section-B shapes: T = 3, rows [3, 500, 40], gradient rows T * D + 8 apart
    with permuted slots. General path: B = 250, bag lengths drawn from
    BWD_LENS (~25 k ids; the 3-row table's runs cross many chunk edges).
    One-hot: B = 256 (a multiple of every chunk size) and B = 250 (of none)."""
    name, B, onehot, bf16, use_psw, mean = BWD_PATHS[path]
    T = 3
    g = _gen(4, D, path)
    if onehot:
        lens = torch.ones(T * B, dtype=torch.int64)
    else:
        lens = torch.tensor(BWD_LENS)[torch.randint(0, len(BWD_LENS), (T * B,), generator=g)]
    return _bwd_case(name, D, T, B, BWD_ROWS, lens, bf16, use_psw, mean)


@functools.lru_cache(maxsize=2)
def bwd_long_case(D):
    """T = 2, rows [3, 5000], B = 1024, 16 ids per bag: ~5460 ids on each row of
    the small table, past COMBINE_LONG (256) chunks at every width."""
    T, B = 2, 1024
    return _bwd_case("long", D, T, B, (3, 5000), torch.full((T * B,), 16, dtype=torch.int64),
                     False, False, False, gscale=0.01)


@functools.lru_cache(maxsize=2)
def bwd_onehot_case(D, B):
    """One id per bag, T = 3, fp32 gradient (the 64-bit-key one-hot shapes)."""
    T = 3
    return _bwd_case("oh", D, T, B, BWD_ROWS, torch.ones(T * B, dtype=torch.int64), False,
                     False, False)


@functools.lru_cache(maxsize=2)
def bwd_multirun_case(D, R=2, B=2048):
    """R runs (virtual tables, run-major) of 3 physical tables sharing rows,
    one id per bag: the world > 1 layout of the per-table sort."""
    rows = (50, 9000, 70000)
    T = R * len(rows)
    return _bwd_case("multirun", D, T, B, rows * R, torch.ones(T * B, dtype=torch.int64), False,
                     False, False, tables=rows)


@functools.lru_cache(maxsize=2)
def bwd_fixed_len_case(D):
    """Fixed bag lengths [1, 7, 3] (T = 3, B = 250) with psw and mean, bf16
    gradient: the keys pass may divide instead of searching (``bag_len``)."""
    T, B, L = 3, 250, [1, 7, 3]
    c = _bwd_case("fixed", D, T, B, BWD_ROWS, torch.tensor(L).repeat_interleave(B), True, True,
                  True)
    c["bag_len"] = torch.tensor(L, dtype=torch.int32)
    return c


def bwd_states(c, opt):
    """Fresh (state1, state2, dense_grad) of a case for one optimizer."""
    return make_states(opt, c["W"].shape[0], c["D"], _gen(5, opt, *c["seed"]))


def bwd_exact(c, opt, states, hyper=None):
    s1, s2, dg = states
    return embedding_opt(c["W"], c["urows"], c["g"], opt, c["hyper"] if hyper is None else hyper,
                         s1, s2, dg, weight_decay=WEIGHT_DECAY)


# ------------------------------------------------------------- interaction
INTER_D = (16, 32, 64, 128, 256)
INTER_F = (2, 3, 17, 32)
INTER_B = (1, 37)


def _tri(F):
    li, lj = torch.tril_indices(F, F, offset=-1)
    return li, lj


def _gather_slots(flat, off, stride, F, D, B):
    ar = torch.arange(B)[:, None]
    cols = torch.arange(D)[None, :]
    return [flat[off[i] + ar * stride[i] + cols] for i in range(1, F)]


@functools.lru_cache(maxsize=4)
def inter_case(D, F, B):
    """bf16 inputs of one interaction case. ``dense`` is columns [8, 8 + D) of
    a wider buffer and holds negatives, +0.0 and -0.0; the gradient slots are
    the forward's in reverse order, 16 elements further apart."""
    g = _gen(6, D, F, B)
    T = F - 1
    P = F * (F - 1) // 2
    dense_buf = torch.randn(B, D + 24, generator=g).abs()
    dense_buf[:, 8::3] = -dense_buf[:, 8::3]
    dense_buf[:, 8 + 1] = 0.0
    dense_buf[:, 8 + 2] = -0.0
    dense_buf[:, 8 + 7] = 0.0
    dense_buf[:, 8 + D - 1] = -0.0
    dense_buf = dense_buf.to(torch.bfloat16)
    emb = torch.randn(B * T * D, generator=g).to(torch.bfloat16)
    off = [0] + [t * D for t in range(T)]
    stride = [0] + [T * D] * T
    dstride_v = T * D + 16
    doff = [0] + [(T - 1 - t) * D + 8 for t in range(T)]
    dstride = [0] + [dstride_v] * T
    ldo = (D + P + 7) // 8 * 8 + 16
    dz = torch.randn(B, ldo, generator=g).to(torch.bfloat16)
    return dict(D=D, F=F, B=B, P=P, dense_buf=dense_buf, emb=emb, off=off, stride=stride,
                doff=doff, dstride=dstride, d_emb_numel=B * dstride_v + 16, ldo=ldo, dz=dz,
                ones_col=D + P + 3)


def inter_dense(c, buf=None):
    buf = c["dense_buf"] if buf is None else buf
    return buf[:, 8:8 + c["D"]]


def interaction_fwd(c, ones_col=-1):
    """-> (exact, bound) [B, ldo]: [dense | strict lower triangle of X X^T | 0]
    (1 in ``ones_col``); the dense copy and the pad have bound 0."""
    D, F, B, P = c["D"], c["F"], c["B"], c["P"]
    X = torch.stack([inter_dense(c).double()] +
                    [r.double() for r in _gather_slots(c["emb"], c["off"], c["stride"], F, D, B)], 1)
    li, lj = _tri(F)
    Z = torch.bmm(X, X.transpose(1, 2))[:, li, lj]
    M = torch.bmm(X.abs(), X.abs().transpose(1, 2))[:, li, lj]
    exact = torch.zeros(B, c["ldo"], dtype=torch.float64)
    bound = torch.zeros_like(exact)
    exact[:, :D] = X[:, 0]
    exact[:, D:D + P] = Z
    bound[:, D:D + P] = U8 * Z.abs() + (D + 2) * U23 * M
    if ones_col >= 0:
        exact[:, ones_col] = 1.0
    return exact, bound


def interaction_bwd(c, relu_mask):
    """-> (dd, dd_bound [B, D], de, de_bound, de_written [d_emb_numel]): S
    symmetric from dZ's triangle with a zero diagonal, dX = S X; the dense slot
    adds dZ[:, :D] and is zero where ``relu_mask`` and x <= 0; the embedding
    slots land through the gradient slot map."""
    D, F, B, P = c["D"], c["F"], c["B"], c["P"]
    X = torch.stack([inter_dense(c).double()] +
                    [r.double() for r in _gather_slots(c["emb"], c["off"], c["stride"], F, D, B)], 1)
    li, lj = _tri(F)
    dz = c["dz"].double()
    S = torch.zeros(B, F, F, dtype=torch.float64)
    S[:, li, lj] = dz[:, D:D + P]
    S[:, lj, li] = dz[:, D:D + P]
    dX = torch.bmm(S, X)
    M = torch.bmm(S.abs(), X.abs())
    dd = dX[:, 0] + dz[:, :D]
    dd_bound = U8 * dd.abs() + (F + 1 + 2) * U23 * (M[:, 0] + dz[:, :D].abs())
    if relu_mask:
        keep = (X[:, 0] > 0).double()
        dd, dd_bound = dd * keep, dd_bound * keep
    n = c["d_emb_numel"]
    de = torch.zeros(n, dtype=torch.float64)
    de_bound = torch.zeros(n, dtype=torch.float64)
    written = torch.zeros(n, dtype=torch.bool)
    ar = torch.arange(B)[:, None]
    cols = torch.arange(D)[None, :]
    for i in range(1, F):
        ix = (c["doff"][i] + ar * c["dstride"][i] + cols).reshape(-1)
        de[ix] = dX[:, i].reshape(-1)
        de_bound[ix] = (U8 * dX[:, i].abs() + (F + 2) * U23 * M[:, i]).reshape(-1)
        written[ix] = True
    return dd, dd_bound, de, de_bound, written


def check_bounded(got, exact, bound, what):
    """|got - exact| <= bound for every element (0 where the bound is 0).
    Returns the worst error / bound ratio."""
    got = got.detach().cpu().double().reshape(exact.shape)
    err = (got - exact).abs()
    bad = ~(err <= bound)
    assert not bool(bad.any()), (what, int(bad.sum()), float(err[bad].max()))
    nz = bound > 0
    return float((err[nz] / bound[nz]).max()) if bool(nz.any()) else 0.0


# ------------------------------------------------- runners (ops.* on ``dev``)
def _to(t, dev):
    return None if t is None else t.to(dev)


def run_fwd(c, dev, out_dtype, use_psw, mean, onehot=False):
    """ops.embedding_bag_fwd of a forward case into a SENTINEL-filled buffer."""
    from tdfo_amd import ops

    out = torch.full((c["B"] * c["out_stride"],), SENTINEL, dtype=out_dtype, device=dev)
    ops.embedding_bag_fwd(c["W"].to(dev), c["ro"].to(dev), c["idx"].to(dev), c["offs"].to(dev),
                          c["out_off"].to(dev), c["T"], c["B"], out, c["out_stride"], mean=mean,
                          psw=c["psw"].to(dev) if use_psw else None, onehot=onehot)
    return out


def bwd_tensors(c, states, dev):
    """Device copies {"W", "s1", "s2", "dg"} a backward may update in place."""
    s1, s2, dg = states
    return dict(W=c["W"].to(dev).clone(), s1=_to(s1, dev), s2=_to(s2, dev), dg=_to(dg, dev))


def bwd_inputs(c, dev):
    return dict(ro=c["ro"].to(dev), idx=c["idx"].to(dev), offs=c["offs"].to(dev),
                goff=c["goff"].to(dev), grad=c["grad"].to(dev), psw=_to(c["psw"], dev))


def run_bwd(c, opt, dev, states, hyper=None, **kw):
    """ops.embedding_bwd of a backward case (weight decay, hyper and strides of
    section B) -> the updated {"W", "s1", "s2", "dg"} on ``dev``."""
    from tdfo_amd import ops

    t = bwd_tensors(c, states, dev)
    i = bwd_inputs(c, dev)
    hyper = (c["hyper"] if hyper is None else hyper).to(dev)
    ops.embedding_bwd(t["W"], i["ro"], i["idx"], i["offs"], i["goff"], c["T"], c["B"], i["grad"],
                      c["stride"], opt, hyper, state1=t["s1"], state2=t["s2"], eps=EPS,
                      beta1=BETA1, beta2=BETA2, weight_decay=WEIGHT_DECAY, mean=c["mean"],
                      psw=i["psw"], dense_grad=t["dg"], **kw)
    return t


def bwd_before(c, states):
    s1, s2, dg = states
    return dict(W=c["W"], s1=s1, s2=s2, dg=dg)


def same_bits(a, b):
    """Two results of bwd_tensors / run_bwd are bit-identical."""
    return all((a[k] is None and b[k] is None) or torch.equal(a[k], b[k]) for k in a)


def run_inter_fwd(c, dev, ones_col=-1):
    from tdfo_amd import ops

    out = torch.full((c["B"], c["ldo"]), SENTINEL, dtype=torch.bfloat16, device=dev)
    ops.interaction_fwd(inter_dense(c, c["dense_buf"].to(dev)), c["emb"].to(dev), c["off"],
                        c["stride"], c["F"], c["D"], out, ones_col)
    return out


def run_inter_bwd(c, dev, relu_mask):
    """-> (d_dense buffer [B, D + 16] whose columns [8, 8 + D) are the slot,
    d_emb), both SENTINEL-filled before the call."""
    from tdfo_amd import ops

    D = c["D"]
    dd_buf = torch.full((c["B"], D + 16), SENTINEL, dtype=torch.bfloat16, device=dev)
    de = torch.full((c["d_emb_numel"],), SENTINEL, dtype=torch.bfloat16, device=dev)
    ops.interaction_bwd(c["dz"].to(dev), inter_dense(c, c["dense_buf"].to(dev)),
                        c["emb"].to(dev), c["off"], c["stride"], c["F"], D, dd_buf[:, 8:8 + D], de,
                        c["doff"], c["dstride"], relu_mask)
    return dd_buf, de


def check_inter_fwd(out, c, ones_col=-1):
    exact, bound = interaction_fwd(c, ones_col)
    got = out.detach().cpu().double()
    D = c["D"]
    assert torch.equal(got[:, :D], exact[:, :D]), "dense passthrough is a copy"
    return check_bounded(got, exact, bound, "interaction fwd")


def check_inter_bwd(dd_buf, de, c, relu_mask):
    D = c["D"]
    dd, dd_bound, e, e_bound, written = interaction_bwd(c, relu_mask)
    buf = dd_buf.detach().cpu().double()
    r0 = check_bounded(buf[:, 8:8 + D], dd, dd_bound, "d_dense")
    assert bool((buf[:, :8] == SENTINEL).all()) and bool((buf[:, 8 + D:] == SENTINEL).all()), \
        "d_dense: a column outside the slot was written"
    got = de.detach().cpu().double()
    assert bool((got[~written] == SENTINEL).all()), "d_emb: a gap between slots was written"
    r1 = check_bounded(got[written], e[written], e_bound[written], "d_emb")
    return max(r0, r1)
