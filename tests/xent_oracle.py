"""float64 oracle of Linear(E -> V) + label-smoothed cross-entropy and the
shared cases of its kernel tests: the wide-hidden kernels (WIDTHS, E = 128 /
256) and the narrow ones (NARROW_WIDTHS, E = 16 / 32 / 64) run the same CASES,
built per width by ``make_case`` / ``oracle_case``.

The oracle materialises the [N, V] logits in fp64, so shapes stay small. It
is written out by hand (no autograd) to be independent of
``ops.reference.linear_xent``:
    z = H W^T + b,  lse_n = logsumexp_v z_nv,
    loss_n = lse_n - (1 - eps) z_{n, y_n} - eps * mean_v z_nv   (0 if ignored)
    dz = (softmax(z) - eps / V - (1 - eps) onehot(y)) / n_valid (0 if ignored)
    dH = dz W,  dW = dz^T H,  db = sum_n dz,  mean = sum_n loss_n / n_valid

Two bounds are asserted against it. BOUND (2e-4 of the tensor's largest
entry, ``rel_err``) is the older, weaker one. The per-row one is the
project's: ``row_err(kernel) <= max(8 x row_err(yardstick), 2^-20)`` with
``row_err`` / ``bound`` of tests/encoder_oracle.py (``assert_within`` below),
on cases whose number of valid tokens is chosen (``make_nv_case``). The
yardstick is the fp32 reference run on the CPU, or, for the 3-pass bf16
kernels of ``linear_xent`` impl 2, their emulation ``emulate_x3``.
"""
import functools
import math

import torch

from tests import encoder_oracle as eo

EPS = 0.1
IGNORE = 0
BOUND = 2e-4          # against the fp64 oracle, every output
NAMES = ("dH", "loss", "dW", "db")

# (V, N, hs): hs scales H (large logits exercise the running-max rescale)
CASES = [(50, 7, 1.0), (130, 65, 1.0), (1000, 320, 1.0), (4099, 1030, 1.0), (5003, 200, 4.0),
         (5003, 200, 12.0), (70001, 320, 1.0)]
WIDTHS = (128, 256)             # linear_xent_mfma.hip
NARROW_WIDTHS = (16, 32, 64)    # linear_xent.hip (16), linear_xent_wide.hip (32 / 64)
# further shapes of the split test
SPLIT_CASES = [(4099, 320), (130, 65)]


def rel_err(a: torch.Tensor, r: torch.Tensor) -> float:
    """max|a - r| / (max|r| + 1e-12), the metric of tests/test_gpu_bert4rec.py"""
    a, r = a.detach().cpu().double(), r.detach().cpu().double()
    return float((a - r).abs().max() / (r.abs().max() + 1e-12))


@functools.lru_cache(maxsize=None)
def make_case(V: int, N: int, hs: float, E: int):
    """CPU fp32 inputs (H, W, b, y); about 60 % of the labels ignored, one
    label at V - 1 and one at 1, and at (4099, 1030) labels on the first and
    last row of an interior 64-row W tile. Cached: treat as read-only."""
    g = torch.Generator().manual_seed(1000 * E + N + V)
    H = torch.randn(N, E, generator=g) * hs
    W = torch.randn(V, E, generator=g) * 0.2
    b = torch.randn(V, generator=g) * 0.1
    y = torch.randint(1, V, (N,), generator=g)
    y[torch.rand(N, generator=g) < 0.6] = IGNORE
    y[0], y[N - 1] = V - 1, 1
    if (V, N) == (4099, 1030):
        y[3], y[700] = 2048, 2048 + 63
    return H, W, b, y


def oracle(H, W, b, y, eps=EPS, ignore=IGNORE, with_terms=False):
    """-> (dH, lossv, dW, db, mean loss), float64; ``with_terms`` appends the
    magnitude of the terms that db sums (see ``db_err``)"""
    H, W, b = H.double(), W.double(), b.double()
    V = W.shape[0]
    valid = y != ignore
    nv = max(1, int(valid.sum()))
    z = H @ W.t() + b
    lse = torch.logsumexp(z, 1)
    yc = torch.where(valid, y, torch.zeros_like(y))       # (an ignore label may be negative)
    zy = z.gather(1, yc.view(-1, 1)).view(-1)
    lossv = torch.where(valid, lse - (1 - eps) * zy - eps * z.mean(1), torch.zeros_like(lse))
    dz = torch.exp(z - lse[:, None]) - eps / V
    dz[torch.arange(len(y)), yc] -= 1 - eps
    dz = dz * valid[:, None] / nv
    out = (dz @ W, lossv, dz.t() @ H, dz.sum(0), lossv.sum() / nv)
    if with_terms:
        # db_v = sum_n p_nv / nv  -  ((1 - eps) c_v + eps n_valid / V) / nv
        pos = (torch.exp(z - lse[:, None]) * valid[:, None]).sum(0) / nv
        out += (2 * pos - out[3],)
    return out


@functools.lru_cache(maxsize=None)
def oracle_case(V: int, N: int, hs: float, E: int):
    """Cached: treat as read-only."""
    return oracle(*make_case(V, N, hs, E))


# ------------------------------------------------- cases with a chosen n_valid
# Every dispatch decision of the kernels hangs on nv, the device-side count of
# valid tokens, so these cases fix it exactly.
LAYOUTS = ("front", "back", "spread")
FAMILIES = ("randn", "hs12", "hot", "fit", "eps0", "ign100")
# E = 16 (linear_xent.hip), V = 1000: (nv, N, layout). ng = ceil(nv / 16) of the
# first 128-token block walks 1 .. 8, the last block holds 1 or 8 groups, nv % 16
# takes 0, 1 and 15, and 96 / 97 / 128 / 129 sit on the 4-tile-ring (NG <= 6)
# and fused-optimizer (nv <= 128) thresholds.
NV16 = (1, 15, 16, 17, 32, 33, 48, 49, 64, 65, 80, 81, 96, 97, 112, 113, 127, 128, 129, 144, 256,
        257)
NV16_V = 1000
NV16_CASES = [(nv, nv + 7, "spread") for nv in NV16] + [(129, 1030, "back"), (129, 300, "front")]
V_EDGES = (3, 16, 17, 32, 48, 64, 4096, 4099, 70001)
V_EDGE_NV = (17, 129)
WIDE_NV, WIDE_V = (1, 63, 64, 65, 128, 129), (5, 255, 256, 257, 1001)          # E = 32 / 64
MFMA_NV, MFMA_V = (1, 63, 64, 65, 129), (31, 32, 33, 63, 64, 65, 1000)         # E = 128 / 256
FAMILY_SHAPE = (1000, 150, 129)      # (V, N, nv) of the input-family cases
NAMES5 = NAMES + ("mean",)
KINDS = {"dH": "row", "loss": "elem", "dW": "row", "db": "elem", "mean": "vec"}


def edge_ignore(V: int) -> int:
    """The ignore label of a V-edge case: IGNORE, except where the first row of
    the last full 16-row tile is row 0 itself (16 <= V < 32): that row has to
    carry a label, so there the ignored tokens are marked -100."""
    return -100 if 16 <= V < 32 else IGNORE


def valid_positions(N: int, nv: int, layout: str) -> torch.Tensor:
    assert 0 <= nv <= N and layout in LAYOUTS
    if layout == "front":
        return torch.arange(nv)
    if layout == "back":
        return torch.arange(N - nv, N)
    return (torch.arange(nv) * N) // max(1, nv)


class NvCase:
    """inputs (H, W, b, y), eps, ignore and the fp64 oracle's outputs"""

    def __init__(self, inputs, eps, ignore):
        self.inputs, self.eps, self.ignore = inputs, eps, ignore
        self.exact = dict(zip(NAMES5 + ("db_terms",),
                              oracle(*inputs, eps=eps, ignore=ignore, with_terms=True)))
        self.nv = int((inputs[3] != ignore).sum())


@functools.lru_cache(maxsize=None)
def make_nv_case(V: int, N: int, nv: int, E: int, layout: str, hs: float = 1.0, eps: float = EPS,
                 ignore: int = IGNORE, family: str = "randn"):
    """CPU fp32 (H, W, b, y) with exactly ``nv`` valid tokens placed by
    ``layout`` among the N. One valid token is labelled V - 1 and (nv >= 2,
    V >= 16) one the first row of the last full 16-row tile; with an ``ignore``
    other than 0 three tokens are labelled 0. Families:
    "randn"; "hot": every valid token carries one label; "fit": the valid
    tokens point along one of 8 axes and W's label rows along the same axes,
    so that p_y > 0.999 (the other rows' dW becomes tiny). Cached: treat as
    read-only."""
    g = torch.Generator().manual_seed(1000 * E + 7 * N + V + 31 * nv + LAYOUTS.index(layout))
    H = torch.randn(N, E, generator=g) * hs
    W = torch.randn(V, E, generator=g) * 0.2
    b = torch.randn(V, generator=g) * 0.1
    lo = 1 if ignore == 0 else 0
    pos = valid_positions(N, nv, layout)
    lab = torch.randint(lo, V, (nv,), generator=g)
    if family == "hot":
        lab[:] = V // 2
    elif family == "fit":
        axes = min(8, E)
        rows = 1 + (torch.arange(axes) * (V - 2)) // axes        # distinct, never 0
        k = torch.arange(nv) % axes
        H[pos] = 0.1 * H[pos]
        H[pos, k] += 4.0
        W[rows] = 0.0
        W[rows, torch.arange(axes)] = 5.0
        lab = rows[k]
    else:
        assert family == "randn", family
        if ignore != 0 and nv >= 5:
            lab[1:4] = 0                 # label 0 is valid: the hit in W's row 0
        if nv >= 1:
            lab[0] = V - 1
        if nv >= 2 and V >= 16:
            lab[nv - 1] = 16 * (V // 16 - 1)
            assert int(lab[nv - 1]) != ignore
    y = torch.full((N,), ignore, dtype=torch.int64)
    y[pos] = lab
    assert int((y != ignore).sum()) == nv
    return H, W, b, y


@functools.lru_cache(maxsize=None)
def nv_case(V: int, N: int, nv: int, E: int, layout: str = "spread", hs: float = 1.0,
            eps: float = EPS, ignore: int = IGNORE, family: str = "randn") -> NvCase:
    """``make_nv_case`` with its oracle. Cached: treat as read-only."""
    return NvCase(make_nv_case(V, N, nv, E, layout, hs, eps, ignore, family), eps, ignore)


@functools.lru_cache(maxsize=None)
def random_case(V: int, N: int, hs: float, E: int) -> NvCase:
    """``make_case`` (validity drawn at random) as an NvCase. Cached: treat as
    read-only."""
    return NvCase(make_case(V, N, hs, E), EPS, IGNORE)


def edge_case(V: int, nv: int, E: int) -> NvCase:
    """A V-edge case: N = nv + 7, layout "spread", ``edge_ignore(V)``"""
    return nv_case(V, nv + 7, nv, E, "spread", ignore=edge_ignore(V))


def family_case(family: str, E: int) -> NvCase:
    """One mid shape per width of each input family."""
    V, N, nv = FAMILY_SHAPE
    kw = {"randn": {}, "hs12": dict(hs=12.0), "hot": dict(family="hot"), "fit": dict(family="fit"),
          "eps0": dict(eps=0.0), "ign100": dict(ignore=-100)}[family]
    return nv_case(V, N, nv, E, "spread", **kw)


# ------------------------------------------------------------ the yardsticks
LOG2E = 1.4426950408889634
LN2 = 0.6931471805599453


def _split(x):
    hi = x.bfloat16().float()
    return hi, (x - hi).bfloat16().float()


def _mm3(a, b, lo=True):
    """a @ b as the 3-pass bf16 MFMA runs it: ah bh + al bh + ah bl, fp32 sums"""
    ah, al = _split(a)
    bh, bl = _split(b)
    if not lo:
        return ah @ bh
    return ah @ bh + al @ bh + ah @ bl


def emulate_x3(H, W, b, y, eps=EPS, ignore=IGNORE, lo=True):
    """The oracle's formulas in float32 with the four products that
    ``linear_xent`` impl 2 runs on the bf16 MFMA replaced by the three-term
    split, operands as in csrc/kernels/linear_xent.hip:
      pass1 (xent_pass1_x3_body): X = W (H log2 e)^T, both split, the bias
        times log2 e added exactly; P = 2^(X - m); O = P W, both split;
      merge (exact f32): lse, z_y, the smoothing term, dH;
      wgrad (xtok3_of, xent_wgrad_tile3): X again from split H log2 e and
        split W; dz = 2^(X - lse log2 e) - eps / V - (1 - eps)[v = y]
        (unscaled); dW = dz^T (H / nv), both split; db = sum dz / nv.
    ``lo=False`` drops the lo terms (plain bf16 products).
    -> (dH, lossv, dW, db, mean), float32"""
    H, W, b = H.float(), W.float(), b.float()
    N, V = H.shape[0], W.shape[0]
    valid = y != ignore
    idx = torch.nonzero(valid).view(-1)
    nv = max(1, int(idx.numel()))
    scale = torch.tensor(1.0 / nv, dtype=torch.float32)
    Hv, yv = H[idx], y[idx]
    Hs = Hv * LOG2E
    X = _mm3(Hs, W.t(), lo) + b * LOG2E                    # log2 units
    m = X.amax(1, keepdim=True)
    P = torch.exp2(X - m)
    tot = P.sum(1)
    O = _mm3(P, W, lo)
    lse = m.view(-1) * LN2 + torch.log(tot)
    Wy = W[yv]
    zy = (Hv * Wy).sum(1) + b[yv]
    cs, bs = W.sum(0), b.sum()
    zmean = (Hv @ cs + bs) / V
    dH, lossv = torch.zeros_like(H), torch.zeros(N)
    lossv[idx] = lse - (1 - eps) * zy - eps * zmean
    dH[idx] = scale * (O / tot[:, None] - (1 - eps) * Wy - eps * cs / V)
    dz = torch.exp2(X - (lse * LOG2E)[:, None]) - eps / V
    dz[torch.arange(idx.numel()), yv] -= 1 - eps
    dW = _mm3(dz.t().contiguous(), Hv * scale, lo)
    db = dz.sum(0) * scale
    return dH, lossv, dW, db, lossv.sum() / nv


def ref_run(case: NvCase, kind: str = "f32"):
    """The yardstick's outputs: ``ops.reference.linear_xent`` in float32 on the
    CPU ("f32"), or the 3-pass emulation ("x3")."""
    H, W, b, y = case.inputs
    if kind == "x3":
        return dict(zip(NAMES5, emulate_x3(H, W, b, y, case.eps, case.ignore)))
    from tdfo_amd.ops import reference as ref

    out = [torch.zeros_like(H), torch.zeros(H.shape[0]), torch.zeros_like(W), torch.zeros_like(b)]
    ref.linear_xent(H, W, b, y, case.eps, case.ignore, *out)
    return dict(zip(NAMES5, out + [out[1].sum() / max(1, case.nv)]))


def db_err(got, exact, terms):
    """row_err of db per element, with one stated exception. db_v is a
    difference, sum_n p_nv / nv against ((1 - eps) c_v + eps nv / V) / nv (c_v
    tokens labelled v), and ``terms`` = the sum of the two. Where every row of
    W expects a label (V small against nv) the two are of one size and an
    element can cancel hundreds of times; fp32 then holds it to an ulp of the
    terms at best, and the fp32 reference's own error on that element is one
    draw of the rounding: at V = 32, nv = 129, E = 256 it moved between 3.9e-6
    and 2.7e-5 over eight orders of its token sum, and between 5.2e-6 and
    3.4e-5 between two host CPUs -- a yardstick that cannot carry a factor 8.
    So an element that lost more than that factor to cancellation is measured
    against terms_v / 8 (the magnitude of what cancels, as
    ``_check_one_candidate`` of tests/test_gpu_xent_rows.py does) instead of
    against |db_v|; every other element exactly as ``row_err`` does, the
    1e-3 max|db| floor included. Kernel and yardstick alike."""
    g, e, t = (x.detach().cpu().double().reshape(-1) for x in (got, exact, terms))
    if not bool(torch.isfinite(g).all()):
        return math.inf
    den = torch.maximum(torch.clamp_min(e.abs(), 1e-3 * float(e.abs().max())), t / eo.FACTOR)
    den = torch.where(den > 0, den, torch.ones_like(den))
    return float(((g - e).abs() / den).max())


def errs(got, exact):
    """{name: row_err}: dH / dW per row, lossv / db per element (``db_err``),
    the mean"""
    out = {k: eo.row_err(got[k], exact[k], KINDS[k]) for k in NAMES5}
    out["db"] = db_err(got["db"], exact["db"], exact["db_terms"])
    return out


_REF_ERR = {}


def ref_err(case: NvCase, kind: str = "f32"):
    """{name: row_err of the yardstick against the oracle}, computed once per
    case and kind and kept with the case (the pattern of encoder_oracle)."""
    key = (id(case), kind)
    if key not in _REF_ERR:
        _REF_ERR[key] = (case, errs(ref_run(case, kind), case.exact))
    return _REF_ERR[key][1]


def yardstick(E: int, impl) -> str:
    """3-pass bf16 family (E = 16, impl 2): its emulation; else exact fp32"""
    return "x3" if E == 16 and impl == 2 else "f32"


def assert_bound(ke, re_, tag, names=NAMES5):
    """print kernel error, yardstick error and their ratio per tensor, then
    assert row_err(kernel) <= max(8 x row_err(yardstick), 2^-20)"""
    bad = []
    for k in names:
        v = ke[k]
        ratio = v / re_[k] if re_[k] > 0 else (math.inf if v > 0 else 0.0)
        print(f"{tag} {k}: kernel={v:.3e} ref={re_[k]:.3e} ratio={ratio:.2f}")
        if not v <= eo.bound(re_[k]):
            bad.append((k, v, re_[k]))
    assert not bad, (tag, bad)


def assert_within(got, case: NvCase, kind: str, tag: str, names=NAMES5):
    """``assert_bound`` of a kernel's [dH, lossv, dW, db, mean] on ``case``
    against the yardstick ``kind``"""
    got = dict(zip(NAMES5, got)) if not isinstance(got, dict) else got
    assert_bound(errs(got, case.exact), ref_err(case, kind), tag, names)
