"""Float64 oracles, bounds, cached seeded inputs, containers and shared checks
for the kernels that close every DLRM / DCN-v2 / TwoTower step: the loss head
(``head_bce``, ``head_reduce``), the deterministic reductions (``reduce_rows``,
``colsum``), the flat optimizer (``dense_optimizer``, ``check_finite``,
``cast_bf16``, ``reduce_adam``), the AUC histogram (``auc_hist``) and the DCN
glue with ``batch_load`` (csrc/kernels/loss.hip, optim.hip, elementwise.hip,
csrc/include/tdfo_reduce_adam.h). Used by the CPU self-check
(test_tail_oracle.py: every case through the fp32 reference behind ``ops.*``
on CPU tensors) and by the GPU kernel tests (test_gpu_tail_oracle.py).

The oracles are plain float64 torch on CPU tensors, nothing from
``tdfo_amd.ops.reference``. Inputs are built once from seeded generators and
cached; callers move copies to their device and never write to a cached tensor.

Containers (tests/dense_oracle.py's): every operand is a view into a larger
NaN-filled parent -- rows before and after and columns past the logical width
where the op takes a row stride, a 16-byte-aligned slice of a longer buffer
where it takes none (integer operands: ``INT_POISON``) -- and every output is
a view into a SENTINEL-filled parent with a ring around it, NaN (integers:
``INT_UNWRITTEN``) where the op must write. "Still NaN" is "not written",
"ring != SENTINEL" is "written outside". In-place outputs (p, m, v, dx0 and
out under accumulate, loss_acc, hist, the flags) hold their values instead.

Two data modes, u23 = 2^-23, u8 = 2^-8.

exact: integers or small dyadic values whose every partial sum in any order is
  representable in fp32; each oracle asserts sum|terms| < 2^24 (2^8 where the
  result lands in bf16) itself. fp32 results must EQUAL the oracle and bf16
  results its round-to-nearest-even. reduce_rows, head_reduce, colsum, the
  reduce half of reduce_adam (``grad``), dense_optimizer's slab segments
  (SGD, lr = 2^-3, grad scale 2^-1), cross_bwd; concat / split / batch_load
  are moves and are always compared bit for bit.

float: randn-based data, per-element bounds. Derived (IEEE fp32 only):
  sum of n terms       n u23 sum|terms| (the doubled first-order bound of
                       dense_oracle.py; any order, fused or not)
  one bf16 rounding    u8 relative, on top of the fp32 bound
  head logits          (K + 2) u23 (sum_k |h w| + |b|): one rounding per
                       product (bf16 x fp32 is not exact), K adds, the bias:
                       2 K + 1 roundings of 2^-24, within the doubled bound
  reduce_rows          bit-equal to ``fixed_order_column_sums`` (the documented
                       order) on the GPU, (rows + 2) u23 sum|terms| for any
                       order (the CPU reference adds rows sequentially). scale:
                       t = fl(sum * scale), out = fl(out + t), both emulated
                       exactly in float64; only ``accumulate`` with a scale
                       that is no power of two may legitimately fuse into one
                       FMA, so that combination accepts exactly two bit
                       patterns per element, the unfused one and fl(out + sum *
                       scale) (``fma_f32``) -- a deviation from plain bit
                       equality, in exact mode too
  colsum               (M + 2) u23 (sum_r |x| + |out|)
  dense_optimizer m/v  m: 4 u23 (|b1 m| + (1 - b1) G), v: 6 u23 (b2 v + (1 - b2)
                       G^2), Adagrad sum: 6 u23 (m + G^2), with G = |g gs| +
                       |wd p| (<= 3 roundings into gg, <= 3 more each)
  SGD                  m: 4 u23 (|mom m| + G); p: lr * that + 3 u23 (|p| + lr |m|)
  slab segments        (S + 1) u23 (|p| + sum_s |slab|) with lr = gs = 1
  cross_bwd            dy = RNE(a * x0) exactly (a bf16 product is exact in
                       fp32); dx0: 3 u23 sum|terms|, then u8
  cast_bf16, p_bf16    bit for bit RNE (``rne_bits``); a NaN stays a NaN;
                       p_bf16 against the p the kernel itself wrote
Measured (an intrinsic whose accuracy is not documented: __expf in the
sigmoid, log1pf, powf in the bias corrections, the 1-ulp sqrt / rcp of
adam_elem): encoder_oracle.py's convention. The yardstick is the error of the
fp32 reference (``ops.*`` on CPU tensors) against the float64 oracle on the
same inputs, per output and per case, normalised by the magnitude named below;
the GPU gets max(FACTOR * yardstick, FLOOR) with that module's FACTOR = 8 and
FLOOR = 2^-20 (they fit: every normalised quantity is O(1) and an fp32 rounding
of it is 2^-24). The margin stands for another, equally legitimate fp32
evaluation order and 1-ulp intrinsics. Never fitted to a GPU output.
  head_bce   everything downstream of the logits is evaluated in float64 AT
             THE LOGITS THE CODE UNDER TEST WROTE (they are checked against
             the derived bound first), so only the intrinsics' error is left:
             dH / (inv_n |w_k|), dw / (inv_n sum_s |h_sk|), db / (inv_n B),
             loss / sum_s (1 + 2 |x_s|); each plus the derived (B + 2) u23
             sum|terms| of its sum and, for dH, the product's and the bf16
             rounding. A masked dH element must be exactly 0.
  Adam(W), Adagrad p   |p_new - exact| / (|p| + |update|). The oracle takes
             beta1, beta2, eps, lr, step, gs, wd as the kernel holds them
             (float32 in the kernels, Python doubles in the CPU reference;
             lr, step, gs float32 in both -- ``holder``), widened: the
             cancellation in 1 - beta^step at small steps is in the oracle.
             One derived term is added: any fp32 evaluation of beta^t rounds it
             (1 ulp: 2^-23 beta^t at worst), and bc = 1 - beta^t magnifies
             that to 2^-23 beta^t / bc relative -- 6e-5 in bc2 at step 2. The
             reference forms bc in double, so its yardstick cannot hold it:
             |update| u23 (b1^t / bc1 + b2^t / (2 bc2)), the 1/2 from the
             square root. It is 3e-5 of the update at step 2 and vanishes as
             t grows; a bc2 taken at step - 1 is off by 41 % at step 2.
auc_hist: counts are exact because the inputs are: interior logits are
  re-verified in float64 to sit >= 0.25 bucket from an edge (1.2e-4 in the
  sigmoid at nb = 2048, a thousand times fp32's error); edge logits (within
  2^-12 bucket of an edge) may fall on either side: the two buckets around
  each edge are checked by their sum, everything else exactly; +-30, +-100,
  +-inf land in bucket 0 / nb - 1. Labels: > 0.5 is positive (0.5 itself is
  not). NaN logits are out of contract (the bucket of a NaN is whatever the
  float -> int conversion gives) and are not tested.
split_features under relu_mask: a killed element must be == 0 (the kernel
  writes +0, the reference x * 0 keeps x's sign); all others bit for bit.

Worst error / bound ratios of the first full MI355X run (float mode; every
exact case equal, no ring touched, every element written), and beside them,
where the bound is measured, the largest reference yardstick over the op's
cases (the normalised error of the fp32 reference, before FACTOR / FLOOR):
  head_bce logits  0.049 (derived)      head_bce dH    0.994, yardstick 1.2e-7
  head_bce dw      0.075, 1.1e-7        head_bce db    0.051, 8.2e-8
  head_bce loss    0.026, 4.0e-8        reduce_rows    bit-equal (FMA case: 2 patterns)
  colsum           0.166 (derived)      cross_bwd      0.996 (derived)
  dense_optimizer  adamw 0.241, 4.9e-6; adam 0.340, 7.5e-7; adagrad 0.232, 1.4e-7;
                   sgd 0.235, sgd0 0.157, slab segments 0.250 (derived)
  reduce_adam      0.326, 4.8e-7
The two ratios just under 1 (dH, cross_bwd dx0) are the bf16 rounding itself:
u8 is reached just above a power of two.
"""
import dataclasses
import functools
import math

import numpy as np
import torch

from tdfo_amd import ops
from tests.dense_oracle import SENTINEL, U8, U23, Slot, _gen, _up, compare, rne_bf16
from tests.encoder_oracle import FACTOR, FLOOR

F64 = torch.float64
NAN = float("nan")
INT_POISON = -(1 << 40)        # integer operands' surroundings
INT_UNWRITTEN = -1             # integer outputs before the op
EXACT_F32 = 2.0 ** 24
BF, F32, I64 = torch.bfloat16, torch.float32, torch.int64
OPT = {"adamw": ops.OPT_ADAMW, "adam": ops.OPT_ADAM, "sgd": ops.OPT_SGD, "sgd0": ops.OPT_SGD,
       "adagrad": ops.OPT_ADAGRAD}


def f32(x):
    """a Python float as the kernels hold it: rounded to float32, widened"""
    return float(np.float32(x))


def bound(ref_e):
    return max(FACTOR * ref_e, FLOOR)


# ------------------------------------------------------------- containers
def vec_slot(n, dtype, lead=16):
    """[n] at a 16-byte aligned offset of a longer buffer"""
    return Slot(lead + n + 16, lead, (n,), (1,), dtype)


def mat_slot(R, C, ld, dtype):
    """[R, C] with pitch ld: >= 2 rows before, 1 after, 16-byte aligned origin"""
    off = _up(2 * ld, 16) + 16
    return Slot(off + (R + 1) * ld + 16, off, (R, C), (ld, 1), dtype)


def put(slot, logical, fill=NAN):
    """CPU parent holding ``logical`` inside ``fill``"""
    p = slot.parent(fill)
    slot.view(p).copy_(logical)
    return p


def fresh(slot, device, init=None, unwritten=NAN):
    """output parent on ``device``: SENTINEL, the view NaN (or ``init``)"""
    p = slot.parent(SENTINEL, device)
    if init is None:
        slot.view(p).fill_(unwritten)
    else:
        slot.view(p).copy_(init)
    return p


def body(slot, parent):
    return slot.view(parent.detach().cpu())


def ring_ok(slot, parent, what):
    r = parent.detach().cpu().clone()
    slot.view(r).fill_(SENTINEL)
    assert bool((r == SENTINEL).all()), f"{what}: written outside its view (ring changed)"


def written(t, what):
    assert not bool(t.double().isnan().any()), f"{what}: an element was never written"


def bits16(t):
    return t.contiguous().view(torch.int16)


def same_bits(got, want, what):
    """bit-for-bit equality of two tensors of one dtype"""
    assert got.dtype == want.dtype and got.shape == want.shape, (what, got.dtype, want.dtype)
    v = {2: torch.int16, 4: torch.int32, 8: torch.int64}[got.element_size()]
    bad = got.contiguous().view(v) != want.contiguous().view(v)
    assert not bool(bad.any()), (f"{what}: bits differ", int(bad.sum()), bad.nonzero()[0].tolist())


def rne_bits(x):
    """float32 tensor -> the int32 bit patterns (0..65535) of its nearest-even
    bf16, by integer arithmetic; NaN -> -1 (any NaN is accepted there)."""
    u = x.contiguous().view(torch.int32).to(I64) & 0xFFFFFFFF
    r = ((u + 0x7FFF + ((u >> 16) & 1)) >> 16) & 0xFFFF
    return torch.where((u & 0x7FFFFFFF) > 0x7F800000, torch.full_like(r, -1), r)


def check_bf16_is_rne(got_bf16, src_f32, what):
    got = bits16(got_bf16.detach().cpu()).to(I64) & 0xFFFF
    want = rne_bits(src_f32.detach().cpu().float())
    nan = want < 0
    is_nan = (got & 0x7FFF) > 0x7F80
    assert bool(is_nan[nan].all()), f"{what}: a NaN did not stay a NaN"
    bad = (got != want) & ~nan
    assert not bool(bad.any()), (f"{what}: not the round-to-nearest-even bf16", int(bad.sum()),
                                 bad.nonzero()[0].tolist())


def fixed_order_column_sums(p, PH=16):
    """The documented order of reduce_rows / head_reduce / reduce_adam in
    fp32: per column, row phase ph sums rows ph, ph + PH, ... into four
    accumulators (groups of four rows, a partial last group into the first),
    combines them as (s0 + s1) + (s2 + s3), then the PH phases are added in
    order. PH = 16 for the 16-column kernel, 4 for the 64-column one."""
    p = p.float()
    n = p.shape[0]
    out = torch.zeros(p.shape[1], dtype=F32)
    for ph in range(PH):
        s = [torch.zeros(p.shape[1], dtype=F32) for _ in range(4)]
        r = ph
        while r + 3 * PH < n:
            for q in range(4):
                s[q] = s[q] + p[r + q * PH]
            r += 4 * PH
        while r < n:
            s[0] = s[0] + p[r]
            r += PH
        out = out + ((s[0] + s[1]) + (s[2] + s[3]))
    return out


def fma_f32(a, b, c):
    """fl32(a * b + c) with ONE rounding, for fp32 tensors a, c and an fp32
    scalar b: the product is exact in float64 (48 bits); the sum is formed by
    TwoSum and, where inexact, rounded to odd in float64, after which the
    rounding to fp32 (53 >= 2 * 24 + 2 bits) is the correct single one."""
    x, y = a.double() * float(b), c.double()
    hi = x + y
    yy = hi - x
    lo = (x - (hi - yy)) + (y - yy)                      # hi + lo == x + y exactly
    bits = hi.view(I64)
    nudge = (lo != 0) & ((bits & 1) == 0)                # inexact and even: take the odd neighbour
    step = torch.where((lo > 0) == (hi > 0), 1, -1)      # towards lo: away from 0 iff same sign
    return torch.where(nudge, bits + step, bits).view(F64).float()


def worst_ratio_line(tag, worst):
    return f"tail-oracle worst error/bound [{tag}]: {worst:.4f}"


def _ratio(err, bnd, what):
    """|err| <= bnd everywhere (NaN fails) -> worst err / bnd"""
    bad = ~(err <= bnd)
    assert not bool(bad.any()), (f"{what}: outside its bound", int(bad.sum()),
                                 bad.nonzero()[0].tolist(), float(err[bad][0]),
                                 float(bnd[bad][0]))
    nz = bnd > 0
    return float((err[nz] / bnd[nz]).max()) if bool(nz.any()) else 0.0


# =================================================================== head_bce
@dataclasses.dataclass(frozen=True)
class HeadCase:
    K: int
    B: int
    relu: bool = True
    sat: bool = False          # w scaled so that logits reach +-100
    frac: bool = False         # labels in [0, 1] instead of {0, 1}


def head_id(c):
    return f"K{c.K}-B{c.B}-{'relu' if c.relu else 'lin'}" + ("-sat" if c.sat else "") \
        + ("-frac" if c.frac else "")


HEAD_KS = (16, 32, 64, 128, 256, 512, 1024)
HEAD_BS = (1, 15, 16, 17, 37)
HEAD_CASES = tuple([HeadCase(K, B, r) for K in HEAD_KS for B in HEAD_BS for r in (True, False)]
                   + [HeadCase(K, 37, True, sat=True) for K in HEAD_KS]
                   + [HeadCase(64, 17, True, frac=True)])
HEAD_WORLD = 3                 # inv_n = 1 / (B * world), as DLRM passes it


@functools.lru_cache(maxsize=None)
def head_data(c):
    g = _gen(11, c.K, c.B, c.relu, c.sat, c.frac)
    K, B = c.K, c.B
    H = torch.randn(B, K, generator=g).bfloat16().double()
    flat, perm = H.view(-1), torch.randperm(B * K, generator=g)
    q = max(1, B * K // 8)
    flat[perm[:q]] = 0.0
    flat[perm[q:2 * q]] = -0.0
    flat[perm[2 * q]] = -1.5
    w = (torch.randn(K, generator=g) / math.sqrt(K)).float().double()
    b = (torch.randn(1, generator=g) * 0.25).float().double()
    if c.sat:                                  # sample 0's logit to about +-100
        dot = float(H[0] @ w)
        w = (w * ((100.0 - float(b) * math.copysign(1.0, dot)) / abs(dot))).float().double()
    x = H @ w + b
    y = torch.randint(0, 2, (B,), generator=g).double()
    if c.frac:
        y = torch.rand(B, generator=g).float().double()
    if c.sat:
        y[0] = 1.0 if float(x[0]) < 0 else 0.0          # the wrong side: loss ~ |x|
        assert abs(float(x[0])) > 95 and float(x.abs().max()) > 89   # exp(89) overflows fp32
    inv_n = f32(1.0 / (B * HEAD_WORLD))
    d = dict(H=H, w=w, b=b, y=y, inv_n=inv_n, x=x, T=H.abs() @ w.abs() + b.abs(),
             nparts=ops.head_parts(B))
    assert bool(((H == 0) & torch.signbit(H)).any()) and bool(((H == 0) & ~torch.signbit(H)).any())
    assert bool((H < 0).any())
    sl = dict(H=mat_slot(B, K, K + 8, BF), w=vec_slot(K, F32), b=vec_slot(1, F32),
              y=vec_slot(B, F32), logits=vec_slot(B, F32), part=vec_slot(d["nparts"] * (K + 2), F32))
    d["slots"] = sl
    d["in"] = {k: put(sl[k], d[k]) for k in ("H", "w", "b", "y")}
    assert torch.equal(body(sl["H"], d["in"]["H"]).double(), H)
    return d


def _dh_slot(c, dtype):
    return mat_slot(c.B, c.K, c.K + 8, dtype)


def run_head(c, device, dh_dtype=BF):
    """ops.head_bce on ``device`` -> output parents on the CPU. dh_dtype fp32
    (CPU only): the reference's dH before its bf16 rounding, for the yardstick."""
    d = head_data(c)
    sl = d["slots"]
    i = {k: sl[k].view(p.to(device)) for k, p in d["in"].items()}
    dhs = _dh_slot(c, dh_dtype)
    o = {"logits": fresh(sl["logits"], device), "dH": fresh(dhs, device),
         "part": fresh(sl["part"], device)}
    ops.head_bce(i["H"], i["w"], i["b"], i["y"], d["inv_n"], c.relu, sl["logits"].view(o["logits"]),
                 dhs.view(o["dH"]), sl["part"].view(o["part"]))
    return {k: p.cpu() for k, p in o.items()}


def head_exact(c, x):
    """everything downstream of the logits ``x`` (float64), exactly"""
    d = head_data(c)
    H, w, y, inv_n = d["H"], d["w"], d["y"], d["inv_n"]
    g = (torch.sigmoid(x) - y) * inv_n
    loss = x.clamp_min(0) - x * y + torch.log1p(torch.exp(-x.abs()))
    live = (H > 0) if c.relu else torch.ones_like(H, dtype=torch.bool)     # +-0.0: not > 0
    dH = torch.where(live, g[:, None] * w[None, :], torch.zeros_like(H))
    return dict(g=g, live=live, dH=dH, dw=(g[:, None] * H).sum(0), db=g.sum(), loss=loss.sum(),
                dw_terms=(g[:, None] * H).abs().sum(0), db_terms=g.abs().sum(),
                loss_terms=(x.clamp_min(0) + (x * y).abs() + math.log(2.0)).sum(),
                mag_dH=inv_n * w.abs()[None, :].expand_as(H), mag_dw=inv_n * H.abs().sum(0),
                mag_db=inv_n * c.B, mag_loss=float((1 + 2 * x.abs()).sum()))


def _head_parts_of(c, got):
    d = head_data(c)
    part = body(d["slots"]["part"], got["part"]).double().view(d["nparts"], c.K + 2)
    return part


def check_head(c, got, yard=None, dh_dtype=BF):
    """``got``: run_head's parents. yard None: measuring mode -- structure and
    the derived logits bound are asserted, the normalised errors of the
    measured quantities are returned. Else {dH, dw, db, loss: yardstick} and
    every bound is asserted; returns {output: worst error / bound}."""
    d = head_data(c)
    sl, B, K = d["slots"], c.B, c.K
    for k, s in (("logits", sl["logits"]), ("dH", _dh_slot(c, dh_dtype)), ("part", sl["part"])):
        ring_ok(s, got[k], f"head_bce {k}")
    x = body(sl["logits"], got["logits"]).double()
    dH = body(_dh_slot(c, dh_dtype), got["dH"]).double()
    part = _head_parts_of(c, got)
    written(x, "head_bce logits")
    written(dH, "head_bce dH")
    written(part, "head_bce part")
    out = {"logits": _ratio((x - d["x"]).abs(), (K + 2) * U23 * d["T"], "head_bce logits")}
    e = head_exact(c, x)
    dead = ~e["live"]
    assert bool((dH[dead] == 0).all()), "head_bce dH: a masked element is not exactly 0"
    s = part.sum(0)
    errs = {"dH": (dH - e["dH"]).abs(), "dw": (s[:K] - e["dw"]).abs(),
            "db": (s[K] - e["db"]).abs().reshape(1), "loss": (s[K + 1] - e["loss"]).abs().reshape(1)}
    mags = {"dH": e["mag_dH"], "dw": e["mag_dw"], "db": torch.tensor([e["mag_db"]], dtype=F64),
            "loss": torch.tensor([e["mag_loss"]], dtype=F64)}
    if yard is None:
        res = {}
        for k in errs:
            nz = mags[k] > 0
            res[k] = float((errs[k][nz] / mags[k][nz]).max()) if bool(nz.any()) else 0.0
        return res
    n = (B + 2) * U23
    bd = {"dH": bound(yard["dH"]) * mags["dH"] + U23 * e["dH"].abs(),
          "dw": bound(yard["dw"]) * mags["dw"] + n * e["dw_terms"],
          "db": bound(yard["db"]) * mags["db"] + n * e["db_terms"].reshape(1),
          "loss": bound(yard["loss"]) * mags["loss"] + n * e["loss_terms"].reshape(1)}
    if dh_dtype == BF:
        bd["dH"] = bd["dH"] + U8 * (e["dH"].abs() + bd["dH"])
    bd["dH"] = torch.where(dead, torch.zeros_like(bd["dH"]), bd["dH"])
    for k in errs:
        out[k] = _ratio(errs[k], bd[k], f"head_bce {k}")
    return out


@functools.lru_cache(maxsize=None)
def head_yard(c):
    """the fp32 reference's normalised errors on this case (dH unrounded)"""
    return check_head(c, run_head(c, "cpu", dh_dtype=F32), None, dh_dtype=F32)


def check_head_chain(c, got, device):
    """the part the op wrote through head_reduce and reduce_rows: grad and the
    loss bit-equal to the documented order, loss_acc +=, the step bumps"""
    d = head_data(c)
    K, nparts = c.K, d["nparts"]
    part = body(d["slots"]["part"], got["part"])
    want = fixed_order_column_sums(part.view(nparts, K + 2), 16)
    ps = d["slots"]["part"]
    pdev = ps.view(got["part"].to(device))
    gs, ls, hs = vec_slot(K + 1, F32), vec_slot(1, F32), vec_slot(3, F32)
    grad = fresh(gs, device)
    lacc = fresh(ls, device, init=torch.tensor([1.5]))
    h1 = fresh(hs, device, init=torch.tensor([0.125, 4.0, 1.0]))
    h2 = fresh(hs, device, init=torch.tensor([0.25, 9.0, 0.5]))
    ops.head_reduce(pdev, nparts, K, gs.view(grad), ls.view(lacc), (hs.view(h1), hs.view(h2)))
    for s, p, nm in ((gs, grad, "grad"), (ls, lacc, "loss_acc"), (hs, h1, "bump"), (hs, h2, "bump")):
        ring_ok(s, p, f"head_reduce {nm}")
    same_bits(body(gs, grad), want[:K + 1], "head_reduce grad")
    same_bits(body(ls, lacc), torch.tensor([1.5]) + want[K + 1:], "head_reduce loss_acc")
    assert body(hs, h1).tolist() == [0.125, 5.0, 1.0] and body(hs, h2).tolist() == [0.25, 10.0, 0.5], \
        "head_reduce: step bumps"
    os_ = vec_slot(K + 2, F32)
    out = fresh(os_, device)
    ops.reduce_rows(pdev, nparts, K + 2, K + 2, os_.view(out), False, 1.0)
    ring_ok(os_, out, "reduce_rows(part)")
    same_bits(body(os_, out), want, "reduce_rows(part)")


# ================================================================ reduce_rows
@dataclasses.dataclass(frozen=True)
class RRCase:
    n: int
    rows: int
    acc: bool = False
    scale: float = 1.0
    pad: int = 8               # ld = n + pad

    @property
    def PH(self):
        return 4 if self.n >= 16384 else 16


def rr_id(c):
    return f"n{c.n}-r{c.rows}-{'acc' if c.acc else 'set'}-s{c.scale:.3g}"


_RR_VARIANTS = ((False, 1.0), (True, 1.0), (False, 0.5), (True, 0.5), (False, 1 / 3), (True, 1 / 3))
_RR_SHAPES = ([(n, r) for n in (1, 15, 16, 17, 16383) for r in (1, 3, 63, 64, 65, 77)]
              + [(n, r) for n in (16384, 16384 + 65) for r in (1, 3, 15, 16, 17, 77)])
RR_CASES = tuple([RRCase(n, r, *_RR_VARIANTS[i % 6]) for i, (n, r) in enumerate(_RR_SHAPES)]
                 + [RRCase(17, 65, a, s) for a, s in _RR_VARIANTS]
                 + [RRCase(16384 + 65, 17, a, s) for a, s in _RR_VARIANTS]
                 + [RRCase(8192 * 64 + 67, 5, True, 0.5)])       # past the 8192-block cap
RR_CASES = tuple(dict.fromkeys(RR_CASES))


@functools.lru_cache(maxsize=64)
def rr_data(c, mode):
    g = _gen(23, c.n, c.rows, c.acc, mode == "float")
    if mode == "exact":
        p = torch.randint(-8, 9, (c.rows, c.n), generator=g).float()
        o0 = torch.randint(-8, 9, (c.n,), generator=g).float()
    else:
        p = torch.randn(c.rows, c.n, generator=g)
        o0 = torch.randn(c.n, generator=g)
    ld = c.n + c.pad
    ps, os_ = mat_slot(c.rows, c.n, ld, F32), vec_slot(c.n, F32)
    return dict(p=p, o0=o0, ld=ld, ps=ps, os=os_, pin=put(ps, p))


def rr_oracle(c, mode):
    """-> (exact float64 result, the documented-order fp32 result, |terms|)"""
    d = rr_data(c, mode)
    sc = f32(c.scale)
    s64 = d["p"].double().sum(0)
    mag = d["p"].double().abs().sum(0)
    fo = fixed_order_column_sums(d["p"], c.PH)
    if mode == "exact":
        assert float(mag.max()) < EXACT_F32 and torch.equal(fo.double(), s64)
    t = (fo.double() * sc).float()                       # one fp32 rounding
    fixed = (d["o0"].double() + t.double()).float() if c.acc else t
    exact = s64 * sc + (d["o0"].double() if c.acc else 0)
    return exact, fixed, mag * sc + (d["o0"].double().abs() if c.acc else 0)


def run_rr(c, mode, device):
    d = rr_data(c, mode)
    par = d["pin"].to(device)
    inp = par[d["ps"].off: d["ps"].off + (c.rows - 1) * d["ld"] + c.n]
    out = fresh(d["os"], device, init=d["o0"] if c.acc else None)
    ops.reduce_rows(inp, c.rows, c.n, d["ld"], d["os"].view(out), c.acc, c.scale)
    return out.cpu()


def check_rr(c, mode, got, bitwise):
    """bitwise: the documented order must hold bit for bit (the GPU kernels);
    else (any order, the CPU reference) the derived bound, equality in exact
    mode with a power-of-two scale."""
    d = rr_data(c, mode)
    ring_ok(d["os"], got, "reduce_rows out")
    o = body(d["os"], got)
    written(o, "reduce_rows out")
    exact, fixed, mag = rr_oracle(c, mode)
    pow2 = math.log2(c.scale).is_integer()
    if c.acc and not pow2 and (bitwise or mode == "exact"):
        # out + sum * scale may be contracted into one FMA: exactly two bit
        # patterns are legitimate, fl(out + fl(sum * scale)) and fl(out + sum * scale)
        fused = fma_f32(fixed_order_column_sums(d["p"], c.PH), f32(c.scale), d["o0"])
        v = torch.int32
        bad = (o.view(v) != fixed.view(v)) & (o.view(v) != fused.view(v))
        assert not bool(bad.any()), ("reduce_rows out: bits differ from the unfused and the fused "
                                     "result", int(bad.sum()), bad.nonzero()[0].tolist())
        return 0.0
    if bitwise or (mode == "exact"):
        same_bits(o, fixed, "reduce_rows out")
        return 0.0
    return _ratio((o.double() - exact).abs(), (c.rows + 2) * U23 * mag, "reduce_rows out")


# ===================================================================== colsum
@dataclasses.dataclass(frozen=True)
class CSCase:
    M: int
    N: int
    acc: bool = False


def cs_id(c):
    return f"{c.M}x{c.N}-{'acc' if c.acc else 'set'}"


CS_CASES = tuple(CSCase(M, N, a) for M in (1, 15, 16, 17, 533) for N in (8, 64, 72, 520)
                 for a in (False, True))


@functools.lru_cache(maxsize=None)
def cs_data(c, mode):
    g = _gen(31, c.M, c.N, mode == "float")
    if mode == "exact":
        x = torch.randint(-3, 4, (c.M, c.N), generator=g).double()
        o0 = torch.randint(-8, 9, (c.N,), generator=g).double()
    else:
        x = torch.randn(c.M, c.N, generator=g).bfloat16().double()
        o0 = torch.randn(c.N, generator=g).float().double()
    xs, os_ = mat_slot(c.M, c.N, c.N + 8, BF), vec_slot(c.N, F32)
    mag = x.abs().sum(0) + (o0.abs() if c.acc else 0)
    if mode == "exact":
        assert float(mag.max()) < EXACT_F32
    return dict(x=x, o0=o0, xs=xs, os=os_, xin=put(xs, x), mag=mag,
                exact=x.sum(0) + (o0 if c.acc else 0))


def run_cs(c, mode, device):
    d = cs_data(c, mode)
    out = fresh(d["os"], device, init=d["o0"] if c.acc else None)
    ops.colsum(d["xs"].view(d["xin"].to(device)), d["os"].view(out), c.acc)
    return out.cpu()


def check_cs(c, mode, got):
    d = cs_data(c, mode)
    ring_ok(d["os"], got, "colsum out")
    return compare(body(d["os"], got), d["exact"], (c.M + 2) * U23 * d["mag"], mode, False,
                   "colsum out")


# ============================================================ dense_optimizer
B1, B2, EPS, LR, MOM = 0.9, 0.999, 1e-8, 0.1, 0.9


@dataclasses.dataclass(frozen=True)
class DOCase:
    opt: str                   # adamw | adam | sgd (momentum 0.9) | sgd0 (m=None) | adagrad
    step: float
    wd: float
    gs: float
    n: int
    bf16: bool = True
    found: "float | None" = None      # found_inf's value, None: not passed


def do_id(c):
    return (f"{c.opt}-t{c.step:g}-wd{c.wd:g}-gs{c.gs:g}-n{c.n}" + ("-bf16" if c.bf16 else "")
            + ("" if c.found is None else f"-inf{c.found:g}"))


DO_OPTS = ("adamw", "adam", "sgd", "sgd0", "adagrad")
DO_GRID_N = 4096 * 256 * 4 + 1028
DO_CASES = tuple(
    [DOCase(o, t, wd, gs, n, bf16=(i + j + k) % 2 == 0)
     for o in DO_OPTS for i, t in enumerate((1.0, 2.0, 5.0, 1e6)) for j, wd in enumerate((0.0, 0.01))
     for k, gs in enumerate((1.0, 0.5)) for n in (4, 4096 + 64)]
    + [DOCase("adamw", 5.0, 0.01, 0.5, DO_GRID_N, bf16=True)]
    + [DOCase(o, 2.0, 0.01, 0.5, 4096 + 64, bf16=True, found=f) for o in DO_OPTS for f in (1.0, 0.0)])
assert len(set(DO_CASES)) == len(DO_CASES)


def _has_m(opt):
    return opt != "sgd0"


def _has_v(opt):
    return opt in ("adamw", "adam")


@functools.lru_cache(maxsize=8)
def do_data(c):
    g = _gen(41, DO_OPTS.index(c.opt), c.n)
    n = c.n
    p = torch.randn(n, generator=g)
    gr = torch.randn(n, generator=g)
    m = torch.randn(n, generator=g) * 0.1
    if c.opt == "adagrad":
        m = m.abs()
    v = torch.rand(n, generator=g) * 0.01
    # planted: g = 0; g = v = 0 with m != 0 (the step is m / (bc1 eps): only a
    # correctly placed eps matches); v ~ 1e-16; a large |g|
    gr[0] = 0.0
    gr[1], v[1], m[1] = 0.0, 0.0, 1e-6
    gr[2], v[2], m[2] = 0.0, 1e-16, 1e-6
    gr[3] = 1e4
    sl = dict(p=vec_slot(n, F32), g=vec_slot(n, F32), m=vec_slot(n, F32), v=vec_slot(n, F32),
              pb=vec_slot(n, BF), hyper=vec_slot(3, F32), found=vec_slot(1, F32))
    pb0 = torch.randn(n, generator=g).bfloat16()
    return dict(p=p, g=gr, m=m, v=v, pb0=pb0, slots=sl, gin=put(sl["g"], gr),
                hyper=torch.tensor([LR, c.step, c.gs], dtype=F32))


def holder(device):
    """how the code under test holds beta1, beta2, eps, wd and the momentum:
    the kernels as float32 arguments, the CPU reference as Python doubles
    (lr, step and the grad scale are float32 on both: they live in ``hyper``)"""
    return f32 if torch.device(device).type == "cuda" else float


def adam_oracle(p, g, m, v, lr, step, gs, wd, adamw, hold=f32):
    """float64 Adam / AdamW of adam_elem, hyper-parameters as the code holds them"""
    b1, b2, eps, wd = hold(B1), hold(B2), hold(EPS), hold(wd)
    lr, gs, step = f32(lr), f32(gs), f32(step)
    gg = g * gs
    G = gg.abs() + wd * p.abs() * (0 if adamw else 1)
    if adamw:
        p1 = p - lr * wd * p
    else:
        gg, p1 = gg + wd * p, p
    m1 = b1 * m + (1 - b1) * gg
    v1 = b2 * v + (1 - b2) * gg * gg
    upd = lr * (m1 / (1 - b1 ** step)) / ((v1 / (1 - b2 ** step)).sqrt() + eps)
    # an fp32 beta^t carries up to 1 ulp (2^-23 beta^t at worst), which 1 - beta^t magnifies
    rel_bc = U23 * (b1 ** step / (1 - b1 ** step) + 0.5 * b2 ** step / (1 - b2 ** step))
    return dict(p=p1 - upd, m=m1, v=v1, mag_p=p.abs() + upd.abs(), bc_p=rel_bc * upd.abs(),
                bm=4 * U23 * ((b1 * m).abs() + (1 - b1) * G),
                bv=6 * U23 * (b2 * v.abs() + (1 - b2) * G * G))


def do_oracle(c, p, g, m, v, hold=f32):
    if _has_v(c.opt):
        return adam_oracle(p, g, m, v, LR, c.step, c.gs, c.wd, c.opt == "adamw", hold)
    lr, gs, wd, step, mom, eps = f32(LR), f32(c.gs), hold(c.wd), f32(c.step), hold(MOM), hold(EPS)
    gg = g * gs + wd * p
    G = (g * gs).abs() + wd * p.abs()
    if c.opt == "adagrad":
        m1 = m + gg * gg
        upd = lr * gg / (m1.sqrt() + eps)
        return dict(p=p - upd, m=m1, mag_p=p.abs() + upd.abs(), bm=6 * U23 * (m.abs() + G * G))
    if c.opt == "sgd":
        m1 = mom * m + gg if step > 1 else gg          # the first step takes the gradient
        bm = 4 * U23 * ((mom * m).abs() * (1 if step > 1 else 0) + G)
        return dict(p=p - lr * m1, m=m1, bm=bm, bp=lr * bm + 3 * U23 * (p.abs() + lr * m1.abs()))
    return dict(p=p - lr * gg, bp=4 * U23 * (p.abs() + lr * G))


def run_do(c, device):
    """-> {p, m, v, pb, found: parents on the CPU}"""
    d = do_data(c)
    sl = d["slots"]
    o = {"p": fresh(sl["p"], device, init=d["p"])}
    if _has_m(c.opt):
        o["m"] = fresh(sl["m"], device, init=d["m"])
    if _has_v(c.opt):
        o["v"] = fresh(sl["v"], device, init=d["v"])
    if c.bf16:
        o["pb"] = fresh(sl["pb"], device, init=d["pb0"] if c.found else None)
    if c.found is not None:
        o["found"] = fresh(sl["found"], device, init=torch.tensor([c.found]))
    hyper = fresh(sl["hyper"], device, init=d["hyper"])
    vw = {k: sl[k].view(t) for k, t in o.items()}
    ops.dense_optimizer(vw["p"], sl["g"].view(d["gin"].to(device)), vw.get("m"), vw.get("v"),
                        vw.get("pb"), OPT[c.opt], sl["hyper"].view(hyper), B1, B2, EPS, c.wd,
                        MOM if c.opt == "sgd" else 0.0, vw.get("found"))
    o["hyper"] = hyper
    return {k: t.cpu() for k, t in o.items()}


def check_do(c, got, yard=None, hold=f32):
    """yard None: measuring mode (returns the normalised p error); else the
    yardstick of p -> worst error / bound over p, m, v. hold: ``holder`` of
    the device that produced ``got``."""
    d = do_data(c)
    sl = d["slots"]
    for k, t in got.items():
        ring_ok(sl[k], t, f"dense_optimizer {k}")
    same_bits(body(sl["hyper"], got["hyper"]), d["hyper"], "dense_optimizer hyper")
    gp = body(sl["p"], got["p"])
    if c.found is not None:
        assert float(body(sl["found"], got["found"])) == c.found, "dense_optimizer: found_inf changed"
    if c.found:
        for k, src in (("p", "p"), ("m", "m"), ("v", "v"), ("pb", "pb0")):
            if k in got:
                same_bits(body(sl[k], got[k]), d[src].to(sl[k].dtype),
                          f"dense_optimizer {k} under found_inf")
        return 0.0
    written(gp, "dense_optimizer p")
    if c.bf16:
        check_bf16_is_rne(body(sl["pb"], got["pb"]), gp, "dense_optimizer p_bf16")
    e = do_oracle(c, d["p"].double(), d["g"].double(), d["m"].double(), d["v"].double(), hold)
    worst = 0.0
    for k, bk in (("m", "bm"), ("v", "bv")):
        if k in got:
            worst = max(worst, _ratio((body(sl[k], got[k]).double() - e[k]).abs(), e[bk],
                                      f"dense_optimizer {k}"))
    err = (gp.double() - e["p"]).abs()
    if "bp" in e:
        return max(worst, _ratio(err, e["bp"], "dense_optimizer p"))
    if yard is None:
        return float((err / e["mag_p"]).max())
    return max(worst, _ratio(err, bound(yard) * e["mag_p"] + e.get("bc_p", 0), "dense_optimizer p"))


@functools.lru_cache(maxsize=None)
def do_yard(c):
    if c.found or not (_has_v(c.opt) or c.opt == "adagrad"):
        return 0.0
    return check_do(c, run_do(c, "cpu"), None, float)


def check_do_flag_zero(opt, device):
    """found_inf = 0 steps exactly as the call without the flag does"""
    flag = DOCase(opt, 2.0, 0.01, 0.5, 4096 + 64, bf16=True, found=0.0)
    assert flag in DO_CASES
    a, b = run_do(flag, device), run_do(dataclasses.replace(flag, found=None), device)
    sl = do_data(flag)["slots"]
    for k in b:
        same_bits(body(sl[k], a[k]), body(sl[k], b[k]), f"dense_optimizer {k}: found_inf = 0 vs none")


# slab segments: (start, length, splits) as in test_dense_optimizer_slab_segments
SLAB_N = 1024
SLAB_SEGS = ((0, 64, 1), (128, 132, 3), (384, 256, 9), (768, 196, 17))


@functools.lru_cache(maxsize=None)
def slab_data(mode):
    g = _gen(43, mode == "float")
    n = SLAB_N

    def draw(*shape):
        if mode == "exact":
            return torch.randint(-4, 5, shape, generator=g).float()
        return torch.randn(shape, generator=g)

    p = draw(n) / (16 if mode == "exact" else 1)
    gr = draw(n)
    slabs = [draw(S, ln) for _, ln, S in SLAB_SEGS]
    gsum, mag = gr.double().clone(), gr.double().abs()
    for (st, ln, S), sb in zip(SLAB_SEGS, slabs):
        gsum[st:st + ln] = sb.double().sum(0)
        mag[st:st + ln] = sb.double().abs().sum(0)
        gr[st:st + ln] = NAN                    # a segment's elements never read g
    lr, gs = (2.0 ** -3, 0.5) if mode == "exact" else (1.0, 1.0)
    if mode == "exact":          # multiples of 2^-4 far below 2^24 * 2^-4: every partial sum exact
        assert float((p.double().abs() + mag).max()) * 16 < EXACT_F32
    terms = torch.full((n,), 2.0, dtype=F64)
    for st, ln, S in SLAB_SEGS:
        terms[st:st + ln] = S + 1
    sl = dict(p=vec_slot(n, F32), g=vec_slot(n, F32), hyper=vec_slot(3, F32),
              slabs=[vec_slot(S * ln, F32) for _, ln, S in SLAB_SEGS])
    return dict(p=p, exact=p.double() - lr * gs * gsum, bnd=terms * U23 * (p.double().abs() + mag),
                hyper=torch.tensor([lr, 3.0, gs]), slots=sl, gin=put(sl["g"], gr),
                sin=[put(s, sb.reshape(-1)) for s, sb in zip(sl["slabs"], slabs)])


def run_slab(mode, device):
    d = slab_data(mode)
    sl = d["slots"]
    p = fresh(sl["p"], device, init=d["p"])
    hyper = fresh(sl["hyper"], device, init=d["hyper"])
    segs = [(st, s.view(t.to(device)), S)
            for (st, _, S), s, t in zip(SLAB_SEGS, sl["slabs"], d["sin"])]
    ops.dense_optimizer(sl["p"].view(p), sl["g"].view(d["gin"].to(device)), None, None, None,
                        ops.OPT_SGD, sl["hyper"].view(hyper), B1, B2, EPS, 0.0, 0.0, None, segs)
    return p.cpu()


def check_slab(mode, got):
    d = slab_data(mode)
    ring_ok(d["slots"]["p"], got, "dense_optimizer(segments) p")
    return compare(body(d["slots"]["p"], got), d["exact"], d["bnd"], mode, False,
                   "dense_optimizer(segments) p")


# ================================================= check_finite and cast_bf16
FLT_MAX = float(np.finfo(np.float32).max)
CF_NS = (1, 63, 64, 65, 4099, 1_100_003)
CF_CASES = tuple([(n, pos, val, start) for n in CF_NS for pos in ("first", "last", "mid")
                  for val, start in (("inf", 0.0), ("-inf", 0.0), ("nan", 0.0))]
                 + [(n, None, None, start) for n in CF_NS for start in (0.0, 1.0)]
                 + [(4099, "mid", "inf", 1.0)])


def cf_id(c):
    return f"n{c[0]}-{c[1]}-{c[2]}-start{c[3]:g}"


def cf_buffer(case):
    n, pos, val, _ = case
    x = torch.randn(n, generator=_gen(51, n))
    edge = torch.tensor([FLT_MAX, -FLT_MAX, 1e-45, -1e-42, -0.0, 0.0])
    x[:min(n, 6)] = edge[:min(n, 6)] if n >= 6 else edge[:1]
    if pos is not None:
        x[{"first": 0, "last": n - 1, "mid": n // 2}[pos]] = float(val)
    return x


def run_cf(case, device):
    xs, fs = vec_slot(case[0], F32), vec_slot(1, F32)
    flag = fresh(fs, device, init=torch.tensor([case[3]]))
    ops.check_finite(xs.view(put(xs, cf_buffer(case)).to(device)), fs.view(flag))
    return flag.cpu()


def check_cf(case, got):
    fs = vec_slot(1, F32)
    ring_ok(fs, got, "check_finite flag")
    want = 1.0 if (case[1] is not None or case[3] == 1.0) else 0.0
    assert float(body(fs, got)) == want, (f"check_finite: flag {float(body(fs, got))}, expected "
                                          f"{want} (only ever set)")


CAST_NS = (1, 255, 257, 1_100_003)
CAST_BITS = (0x3F808000, 0x3F818000, 0xBF808000, 0xBF818000,     # ties: to even down / up
             0x7F7FFFFF, 0xFF7FFFFF,                             # largest finite -> inf
             0x7F800000, 0xFF800000, 0x7FC00000, 0x7F800001, 0xFFFFFFFF,   # inf, NaNs
             0x00000000, 0x80000000, 0x00000001, 0x00008000, 0x00018000, 0x807FFFFF,
             0x3F807FFF, 0x3F808001)                             # just below / above a tie


def cast_input(n):
    x = torch.randn(n, generator=_gen(53, n))
    sp = torch.tensor(np.array(CAST_BITS, dtype=np.uint32).view(np.float32))
    if n >= len(CAST_BITS):
        x[-len(CAST_BITS):] = sp                # the tail: the last, partial block
        x[:len(CAST_BITS)] = sp
    else:
        x[:n] = sp[:n]
    return x


def run_cast(n, device):
    xs, ys = vec_slot(n, F32), vec_slot(n, BF)
    y = fresh(ys, device)
    ops.cast_bf16(xs.view(put(xs, cast_input(n)).to(device)), ys.view(y))
    return y.cpu()


def check_cast(n, got):
    ys = vec_slot(n, BF)
    ring_ok(ys, got, "cast_bf16 out")
    check_bf16_is_rne(body(ys, got), cast_input(n), "cast_bf16 out")


# =================================================================== auc_hist
@dataclasses.dataclass(frozen=True)
class AHCase:
    nb: int
    n: int
    kind: str = "interior"     # interior | edge | sat


def ah_id(c):
    return f"nb{c.nb}-n{c.n}-{c.kind}"


AH_NBS = (1, 2, 199, 200, 512, 2048)
AH_NS = (1, 255, 256, 257, 1024 * 256 + 3)
AH_CASES = tuple([AHCase(nb, n) for nb in AH_NBS for n in AH_NS]
                 + [AHCase(nb, 1500, "edge") for nb in AH_NBS[1:]]
                 + [AHCase(nb, 600, "sat") for nb in AH_NBS])
HALF_UP = float(np.nextafter(np.float32(0.5), np.float32(1)))


def ah_edges(nb):
    return [1] if nb == 2 else list(range(nb // 4, 3 * nb // 4, 3))


@functools.lru_cache(maxsize=None)
def ah_data(c):
    g = _gen(61, c.nb, c.n, ("interior", "edge", "sat").index(c.kind))
    nb, n = c.nb, c.n
    y = torch.randint(0, 2, (n,), generator=g).float()
    if n >= 4:
        y[1], y[2] = 0.5, HALF_UP                      # 0.5 is not > 0.5; the next float is
    pos = y.double() > 0.5
    d = dict(y=y, pos=pos, pair=[])
    if c.kind == "interior":
        b = torch.randint(0, nb, (n,), generator=g)
        p = (b.double() + 0.5 + (torch.rand(n, generator=g).double() - 0.5) * 0.48) / nb
        x = torch.log(p / (1 - p)).float()
        q = torch.sigmoid(x.double()) * nb
        assert bool((q.floor() == b).all()) and bool(((q - b) >= 0.25).all()) \
            and bool(((q - b) <= 0.75).all()), "auc_hist inputs: an element is near a bucket edge"
    elif c.kind == "edge":
        ed = torch.tensor(ah_edges(nb), dtype=I64)
        e = ed[torch.randint(0, len(ed), (n,), generator=g)]
        x = torch.log(e.double() / (nb - e.double())).float()
        q = torch.sigmoid(x.double()) * nb
        assert bool(((q - e).abs() < 2.0 ** -12).all()), "auc_hist inputs: not on an edge"
        b = e                                           # counted at the upper bucket
        d["pair"] = ed.tolist()
    else:
        vals = torch.tensor([30.0, -30.0, 100.0, -100.0, math.inf, -math.inf])
        x = vals[torch.arange(n) % 6]
        b = torch.where(x > 0, nb - 1, 0)
    h0 = (torch.arange(2 * nb, dtype=I64) * 7) % 11 + 1        # accumulated into
    want = h0.clone()
    want[:nb] += torch.bincount(b[~pos], minlength=nb)
    want[nb:] += torch.bincount(b[pos], minlength=nb)
    d.update(x=x, h0=h0, want=want, xs=vec_slot(n, F32), hs=vec_slot(2 * nb, I64),
             npos=int(pos.sum()))
    d["xin"], d["yin"] = put(d["xs"], x), put(d["xs"], y)
    return d


def run_ah(c, device):
    d = ah_data(c)
    h = fresh(d["hs"], device, init=d["h0"])
    ops.auc_hist(d["xs"].view(d["xin"].to(device)), d["xs"].view(d["yin"].to(device)), c.nb,
                 d["hs"].view(h))
    return h.cpu()


def check_hist(got, want, nb, pair, what="auc_hist"):
    """counts equal, except that the two buckets around each edge in ``pair``
    are compared by their sum (per class)"""
    got, want = got.clone().view(2, nb), want.clone().view(2, nb)
    assert bool((got.sum(1) == want.sum(1)).all()), \
        f"{what}: per-class totals {got.sum(1).tolist()} != {want.sum(1).tolist()}"
    for e in pair:
        for t in (got, want):
            t[:, e] += t[:, e - 1]
            t[:, e - 1] = 0
    bad = got != want
    assert not bool(bad.any()), (f"{what}: counts differ", int(bad.sum()), bad.nonzero()[0].tolist())


def check_ah(c, got):
    d = ah_data(c)
    ring_ok(d["hs"], got, "auc_hist hist")
    check_hist(body(d["hs"], got), d["want"], c.nb, d["pair"])


# ================================================================ reduce_adam
@dataclasses.dataclass(frozen=True)
class RACase:
    nparts: int
    n: int
    adamw: bool = True
    nb: int = 0                # 0: no histogram
    nlog: int = 0


def ra_id(c):
    return f"r{c.nparts}-n{c.n}-{'adamw' if c.adamw else 'adam'}-nb{c.nb}-l{c.nlog}"


RA_NPARTS = (1, 15, 16, 17, 63, 64, 65, 511, 512, 513, 600)
_RA_VAR = ((True, 0, 0), (False, 199, 1), (True, 512, 1000), (False, 0, 0), (True, 199, 1000),
           (False, 512, 1))
RA_CASES = tuple([RACase(r, n, *_RA_VAR[(i + j) % 6]) for i, r in enumerate(RA_NPARTS)
                  for j, n in enumerate((15, 16, 2400))]
                 + [RACase(65, 16, *v) for v in _RA_VAR] + [RACase(513, 15, *v) for v in _RA_VAR])
RA_CASES = tuple(dict.fromkeys(RA_CASES))
RA_STEP, RA_WD, RA_GS = 3.0, 0.01, 0.5


@functools.lru_cache(maxsize=32)
def ra_data(c, mode):
    g = _gen(71, c.nparts, c.n, mode == "float")
    n, ld = c.n, c.n + 32
    if mode == "exact":
        part = torch.randint(-4, 5, (c.nparts, n + 1), generator=g).float()
    else:
        part = torch.randn(c.nparts, n + 1, generator=g) * 0.1
    mag = part.double().abs().sum(0)
    fo = fixed_order_column_sums(part, 16)
    if mode == "exact":
        assert float(mag.max()) < EXACT_F32 and torch.equal(fo.double(), part.double().sum(0))
    sl = dict(part=mat_slot(c.nparts, n + 1, ld, F32), grad=vec_slot(n + 1, F32),
              p=vec_slot(n, F32), m=vec_slot(n, F32), v=vec_slot(n, F32), hyper=vec_slot(3, F32),
              loss=vec_slot(1, F64))
    d = dict(part=part, mag=mag, fixed=fo, ld=ld, slots=sl, pin=put(sl["part"], part),
             p=torch.randn(n, generator=g), m=torch.randn(n, generator=g) * 0.1,
             v=torch.rand(n, generator=g) * 0.01, hyper=torch.tensor([LR, RA_STEP, RA_GS]),
             loss0=torch.tensor([1024.0], dtype=F64))
    if c.nb:
        d["ah"] = ah_data(AHCase(c.nb, c.nlog, "interior"))
    return d


def run_ra(c, mode, device, separate=False):
    """ops.reduce_adam, or (separate) reduce_rows + dense_optimizer +
    auc_hist + the loss add on the same containers -> parents on the CPU"""
    d = ra_data(c, mode)
    sl, n = d["slots"], c.n
    par = d["pin"].to(device)
    part = par[sl["part"].off: sl["part"].off + (c.nparts - 1) * d["ld"] + n + 1]
    o = {"grad": fresh(sl["grad"], device), "loss": fresh(sl["loss"], device, init=d["loss0"]),
         "hyper": fresh(sl["hyper"], device, init=d["hyper"])}
    for k in ("p", "m", "v"):
        o[k] = fresh(sl[k], device, init=d[k])
    vw = {k: sl[k].view(t) for k, t in o.items()}
    lg = lb = hv = None
    if c.nb:
        a = d["ah"]
        o["hist"] = fresh(a["hs"], device, init=a["h0"])
        lg, lb = a["xs"].view(a["xin"].to(device)), a["xs"].view(a["yin"].to(device))
        hv = a["hs"].view(o["hist"])
    if not separate:
        ops.reduce_adam(part, c.nparts, n, d["ld"], vw["grad"], vw["p"], vw["m"], vw["v"],
                        vw["hyper"], B1, B2, EPS, RA_WD, c.adamw, vw["loss"], lg, lb, c.nb, hv)
    else:
        ops.reduce_rows(part, c.nparts, n + 1, d["ld"], vw["grad"], False, 1.0)
        vw["loss"] += vw["grad"][n:n + 1].double()
        n4 = _up(n, 4)                      # the flat optimizer steps whole float4s
        pad = {k: torch.zeros(n4, device=device) for k in ("p", "m", "v", "g")}
        for k in ("p", "m", "v"):
            pad[k][:n] = vw[k]
        pad["g"][:n] = vw["grad"][:n]
        ops.dense_optimizer(pad["p"], pad["g"], pad["m"], pad["v"], None,
                            ops.OPT_ADAMW if c.adamw else ops.OPT_ADAM, vw["hyper"], B1, B2, EPS,
                            RA_WD, 0.0, None)
        for k in ("p", "m", "v"):
            vw[k].copy_(pad[k][:n])
        if c.nb:
            ops.auc_hist(lg, lb, c.nb, hv)
    return {k: t.cpu() for k, t in o.items()}


def _ra_slot(d, k):
    return d["ah"]["hs"] if k == "hist" else d["slots"][k]


def check_ra_same(c, mode, fused, sep):
    """the promise of loss.hip: bit-identical to the separate launches"""
    d = ra_data(c, mode)
    for k in fused:
        same_bits(body(_ra_slot(d, k), fused[k]), body(_ra_slot(d, k), sep[k]),
                  f"reduce_adam {k} vs separate launches")


def check_ra(c, mode, got, bitwise, yard=None, hold=f32):
    """against the float64 oracle. yard None: measuring mode -> normalised p
    error; else worst error / bound."""
    d = ra_data(c, mode)
    sl, n = d["slots"], c.n
    for k, t in got.items():
        ring_ok(_ra_slot(d, k), t, f"reduce_adam {k}")
    same_bits(body(sl["hyper"], got["hyper"]), d["hyper"], "reduce_adam hyper")
    grad = body(sl["grad"], got["grad"])
    written(grad, "reduce_adam grad")
    s64 = d["part"].double().sum(0)
    worst = 0.0
    if bitwise or mode == "exact":
        same_bits(grad, d["fixed"], "reduce_adam grad")
    else:
        worst = _ratio((grad.double() - s64).abs(), (c.nparts + 2) * U23 * d["mag"],
                       "reduce_adam grad")
    # loss_acc (fp64) += the fp32 column sum: one fp32 rounding of that sum
    dl = float(body(sl["loss"], got["loss"])) - 1024.0
    lb = 2.0 ** -24 * abs(float(s64[n])) + (0 if mode == "exact" else
                                            (c.nparts + 2) * U23 * float(d["mag"][n]))
    assert abs(dl - float(s64[n])) <= lb, ("reduce_adam loss_acc", dl, float(s64[n]), lb)
    if c.nb:
        a = d["ah"]
        check_hist(body(a["hs"], got["hist"]), a["want"], c.nb, [], "reduce_adam hist")
    # the Adam half from the gradient the op itself reduced
    e = adam_oracle(d["p"].double(), grad[:n].double(), d["m"].double(), d["v"].double(), LR,
                    RA_STEP, RA_GS, RA_WD, c.adamw, hold)
    for k, bk in (("m", "bm"), ("v", "bv")):
        worst = max(worst, _ratio((body(sl[k], got[k]).double() - e[k]).abs(), e[bk],
                                  f"reduce_adam {k}"))
    err = (body(sl["p"], got["p"]).double() - e["p"]).abs()
    if yard is None:
        return float((err / e["mag_p"]).max())
    return max(worst, _ratio(err, bound(yard) * e["mag_p"] + e["bc_p"], "reduce_adam p"))


@functools.lru_cache(maxsize=None)
def ra_yard(c, mode):
    return check_ra(c, mode, run_ra(c, mode, "cpu"), False, None, float)


# ======================================================= DCN glue, batch_load
GLUE_SHAPES = ((1, 16), (5, 64), (27, 128), (32, 16))
GLUE_CASES = tuple((F, D, B) for F, D in GLUE_SHAPES for B in (1, 37))


def _slot_map(F, D, B):
    """distinct offsets and strides per feature, gaps between the regions"""
    off, stride, at = [0], [0], 16
    for i in range(1, F):
        st = D * (1 + i % 3) + 8 * (i % 2)
        off.append(at)
        stride.append(st)
        at += (B - 1) * st + D + 8 * (1 + i % 2)
    return off, stride, at + 16


@functools.lru_cache(maxsize=None)
def glue_data(F, D, B):
    g = _gen(81, F, D, B)
    off, stride, total = _slot_map(F, D, B)
    dense = torch.randn(B, D, generator=g).bfloat16()
    fl, perm = dense.view(-1), torch.randperm(B * D, generator=g)
    q = max(1, B * D // 6)
    fl[perm[:q]] = 0.0
    fl[perm[q:2 * q]] = -0.0
    fl[perm[2 * q]] = -2.0
    feats = torch.randn(B, F, D, generator=g).bfloat16()       # the concatenated row
    feats[:, 0] = dense
    emb = torch.full((total,), NAN, dtype=BF)
    for i in range(1, F):
        emb.as_strided((B, D), (stride[i], 1), off[i]).copy_(feats[:, i])
    dx = torch.randn(B, F, D, generator=g).bfloat16()
    ds = mat_slot(B, D, D + 24, BF)
    return dict(off=off, stride=stride, total=total, dense=dense, feats=feats, emb=emb, dx=dx,
                ds=ds, din=put(ds, dense), outs=vec_slot(B * F * D, BF),
                dx1=vec_slot(B * F * D, BF), dx2=mat_slot(B, F * D, F * D + 16, BF))


def run_concat(F, D, B, device):
    d = glue_data(F, D, B)
    out = fresh(d["outs"], device)
    ops.concat_features(d["ds"].view(d["din"].to(device)), d["emb"].to(device), d["off"],
                        d["stride"], F, D, d["outs"].view(out).view(B, F * D))
    return out.cpu()


def check_concat(F, D, B, got):
    d = glue_data(F, D, B)
    ring_ok(d["outs"], got, "concat_features out")
    o = body(d["outs"], got)
    written(o, "concat_features out")
    same_bits(o, d["feats"].reshape(-1), "concat_features out")


def run_split(F, D, B, relu, pitched, device):
    d = glue_data(F, D, B)
    s = d["dx2"] if pitched else d["dx1"]
    dxin = put(s, d["dx"].reshape(B, F * D) if pitched else d["dx"].reshape(-1)).to(device)
    dd = fresh(d["ds"], device)
    de = torch.full((d["total"],), SENTINEL, dtype=BF, device=device)
    for i in range(1, F):
        de.as_strided((B, D), (d["stride"][i], 1), d["off"][i]).fill_(NAN)
    ops.split_features(s.view(dxin), F, D, d["ds"].view(d["din"].to(device)), d["ds"].view(dd), de,
                       d["off"], d["stride"], relu)
    return dd.cpu(), de.cpu()


def check_split(F, D, B, relu, got):
    d = glue_data(F, D, B)
    dd, de = got
    ring_ok(d["ds"], dd, "split_features d_dense")
    o = body(d["ds"], dd)
    written(o, "split_features d_dense")
    dead = ~(d["dense"].double() > 0) if relu else torch.zeros(B, D, dtype=torch.bool)
    assert bool((o[dead] == 0).all()), "split_features d_dense: a masked element is not 0"
    same_bits(torch.where(dead, torch.zeros_like(o), o),
              torch.where(dead, torch.zeros_like(o), d["dx"][:, 0]), "split_features d_dense")
    rest = de.clone()
    for i in range(1, F):
        v = de.as_strided((B, D), (d["stride"][i], 1), d["off"][i])
        written(v, f"split_features d_emb slot {i}")
        same_bits(v, d["dx"][:, i], f"split_features d_emb slot {i}")
        rest.as_strided((B, D), (d["stride"][i], 1), d["off"][i]).fill_(SENTINEL)
    assert bool((rest == SENTINEL).all()), "split_features d_emb: written between the slots"


CROSS_NS = (8, 2048 * 8 + 8)
CROSS_CASES = tuple((n, a, r) for n in CROSS_NS for a in (False, True) for r in (False, True))


@functools.lru_cache(maxsize=None)
def cross_data(n, mode):
    g = _gen(91, n, mode == "float")

    def draw():
        if mode == "exact":
            return torch.randint(-3, 4, (n,), generator=g).double()
        return torch.randn(n, generator=g).bfloat16().double()

    d = {k: draw() for k in ("dout", "x0", "y", "dx0")}
    d["s"] = vec_slot(n, BF)
    d["in"] = {k: put(d["s"], d[k]) for k in ("dout", "x0", "y")}
    return d


def run_cross(n, acc, add, mode, device):
    d = cross_data(n, mode)
    s = d["s"]
    dy = fresh(s, device)
    dx0 = fresh(s, device, init=d["dx0"] if acc else None)
    i = {k: s.view(p.to(device)) for k, p in d["in"].items()}
    ops.cross_bwd(i["dout"], i["x0"], i["y"], s.view(dy), s.view(dx0), acc, add)
    return dy.cpu(), dx0.cpu()


def check_cross(n, acc, add, mode, got):
    d = cross_data(n, mode)
    s, a = d["s"], d["dout"]
    ring_ok(s, got[0], "cross_bwd dy")
    ring_ok(s, got[1], "cross_bwd dx0")
    compare(body(s, got[0]), a * d["x0"], None, "exact", True, "cross_bwd dy")   # always RNE
    terms = [a * d["y"]] + ([d["dx0"]] if acc else []) + ([a] if add else [])
    ex, mag = sum(terms), sum(t.abs() for t in terms)
    if mode == "exact":
        assert float(mag.max()) < 2.0 ** 8
    b = 3 * U23 * mag
    return compare(body(s, got[1]), ex, b + U8 * (ex.abs() + b), mode, True, "cross_bwd dx0")


BL_CASES = tuple((B, nd, ni) for B in (1, 1000) for nd in (1, 13) for ni in (1, 6, 7))


@functools.lru_cache(maxsize=None)
def bl_data(B, nd, ni):
    g = _gen(95, B, nd, ni)
    dense = torch.randn(B, nd, generator=g) * 5
    dense.view(-1)[0] = 1.00390625                 # a tie: 1 + 2^-8 -> 1.0
    ids = torch.randint(0, 1 << 40, (ni,), generator=g)
    label = torch.randint(0, 2, (B,), generator=g).float()
    sl = dict(dense=mat_slot(B, nd, nd + 3, F32), x0=mat_slot(B, nd + 3, 32, BF),
              ids=vec_slot(ni, I64), label=vec_slot(B, F32))
    return dict(dense=dense, ids=ids, label=label, slots=sl, din=put(sl["dense"], dense),
                iin=put(sl["ids"], ids, fill=INT_POISON), lin=put(sl["label"], label))


def run_bl(B, nd, ni, device):
    d = bl_data(B, nd, ni)
    sl = d["slots"]
    x0 = fresh(sl["x0"], device)
    sl["x0"].view(x0)[:, nd:] = SENTINEL                      # columns past nd are not the op's
    idd = fresh(sl["ids"], device, unwritten=INT_UNWRITTEN)
    lbd = fresh(sl["label"], device)
    args = (sl["dense"].view(d["din"].to(device)), sl["x0"].view(x0),
            sl["ids"].view(d["iin"].to(device)), sl["ids"].view(idd),
            sl["label"].view(d["lin"].to(device)), sl["label"].view(lbd))
    if torch.device(device).type == "cuda":
        torch.ops.tdfo.batch_load(*args)           # the kernel itself, not ops' copy fallback
    else:
        ops.batch_load(*args)
    return x0.cpu(), idd.cpu(), lbd.cpu()


def check_bl(B, nd, ni, got):
    d = bl_data(B, nd, ni)
    sl = d["slots"]
    x0, idd, lbd = got
    ring_ok(sl["ids"], idd, "batch_load ids")
    ring_ok(sl["label"], lbd, "batch_load label")
    assert bool((body(sl["ids"], idd) != INT_UNWRITTEN).all()), "batch_load ids: an element was never written"
    same_bits(body(sl["ids"], idd), d["ids"], "batch_load ids")
    written(body(sl["label"], lbd), "batch_load label")
    same_bits(body(sl["label"], lbd), d["label"], "batch_load label")
    xb = body(sl["x0"], x0)
    written(xb[:, :nd], "batch_load x0")
    check_bf16_is_rne(xb[:, :nd], d["dense"], "batch_load x0")
    r = x0.clone()
    sl["x0"].view(r)[:, :nd] = SENTINEL
    assert bool((r == SENTINEL).all()), "batch_load x0: written outside its view (ring changed)"


CASE_LISTS = {"head": HEAD_CASES, "reduce_rows": RR_CASES, "colsum": CS_CASES, "dense": DO_CASES,
              "check_finite": CF_CASES, "cast": CAST_NS, "auc": AH_CASES, "reduce_adam": RA_CASES,
              "glue": GLUE_CASES, "cross": CROSS_CASES, "batch_load": BL_CASES}
