"""Float64 oracles, per-element error bounds, cached inputs and shared checks
for the bf16 GEMM (``ops.gemm`` and its wrappers), used by the CPU self-check
(test_dense_oracle.py) and by the GPU kernel tests (test_gpu_gemm_oracle.py).

The oracle is plain float64 torch on CPU tensors: no kernels and nothing from
``tdfo_amd.ops.reference``. Every input is built once on the CPU from a seeded
generator and cached; callers move copies to their device and never write to
a cached tensor. ``run_gemm`` / ``run_pair`` call ``ops.gemm`` on a chosen
device (CPU: the fp32 reference, GPU: the HIP kernels) and ``check_gemm``
holds the assertions both share.

Contract checked (csrc/include/tdfo_kernels.h): x = sum_k a_k b_k (+ bias),
v = x, ReLU'd, then zeroed where not (mask > 0) (so -0.0, +0.0, NaN and
negative mask values all kill the element, the smallest subnormal keeps it);
C32 = v, C = bf16(v), C2 = bf16(v * mul + add) from the unrounded v. With
split-K the slabs sum to v; which K range a slab covers is not part of the
contract and is not modelled, except that a slab no K tile is left for
(slab z with z * ceil(ktiles / S) >= ktiles) holds zeros. With ``csum`` the
slabs' column ``csum_col`` sums to sum_k a_k of the row.

Containers. Every operand is a view into a larger NaN-filled parent (rows
before and after, columns past the logical width), so a read outside the
operand that reaches a result shows up as NaN. Every output is a view into a
parent filled with SENTINEL with a ring around it; the elements the op must
write start as NaN, so "still NaN" is "not written" and "ring != SENTINEL" is
"written outside".

Two data modes.

exact: A, B, mul, add hold integers in [-3, 3], bias multiples of 1/4 in
  [-4, 4], K <= 448. Every product, every partial sum in any order, x, v and
  v * mul + add is then a multiple of 1/4 below 2^22 in magnitude, i.e.
  representable in fp32 (24 bits), whatever order or tree the hardware adds
  in and whether or not the multiply-add is fused. So fp32 outputs must EQUAL
  the oracle (``==``, so -0.0 == 0.0) and bf16 outputs must equal its
  round-to-nearest-even. ``gemm_oracle`` asserts the 2^22 limit on
  T = sum|a_k b_k| + |bias| (which bounds every partial sum) and on |C2|.

float: randn operands rounded to bf16. Bounds (u23 = 2^-23, u8 = 2^-8; none
  measured on the code under test), T = sum_k |a_k b_k| + |bias|:
    acc  = (K + S + 2) u23 T. A sequential fp32 sum of n terms is within
           (n - 1) 2^-24 sum|terms| of exact (Higham, to first order), any
           other order is no worse; products of bf16 pairs are exact in fp32.
           K products + bias + the S - 1 additions of the slab sum give
           n <= K + S + 1; the bound is twice that, as in sparse_oracle.py,
           because the MFMA's internal accumulation order and rounding are
           not documented (it also covers a kernel that adds two half-K sums
           at the end). ReLU and the mask are 1-Lipschitz, so |v - v_exact|
           <= acc as well; an element the mask kills must be exactly 0.
    C32  within acc
    C    within acc + u8 (|v| + acc): one round-to-nearest-even into bf16
         (relative 2^-8 at worst, just above a power of two) of a value
         within acc of v.
    C2   e2 = |mul| acc + 2 u23 (|v mul| + |add|): the error of v scaled,
         plus one fp32 rounding each for the multiply and the add (2^-24
         each, doubled); then e2 + u8 (|C2| + e2) for the bf16 rounding.
    csum within (K + S + 2) u23 sum_k |a_k| (same argument, products by 1).
    linear_wgrad  the slabs are summed in fp32 by reduce_rows: those are the
         S - 1 additions acc already counts, so the result is within acc.
         With accumulate the old ``out`` is one more term of the same sum:
         n <= K + S + 2 terms of total magnitude T + |init|, so within
         (K + S + 3) u23 (T + |init|).
"""
import dataclasses
import functools

import torch

from tdfo_amd import ops

U23 = 2.0 ** -23
U8 = 2.0 ** -8
SENTINEL = 7.0
EXACT_LIMIT = 2.0 ** 22
EXACT_MAX_K = 448
BF16_MIN_SUBNORMAL = 2.0 ** -133
# (mask > 0) is False for the first four and for every zero after them; half
# the table is zeros (a ReLU output), a third of it keeps the element
MASK_TABLE = (-2.0, -0.0, 0.0, float("nan"), BF16_MIN_SUBNORMAL, 1.0, 3.0, -0.0, 0.0, 0.0, -0.0,
              1.0)


def _up(x, m):
    return (x + m - 1) // m * m


def _gen(*seed):
    s = 0
    for v in seed:
        s = s * 1000003 + int(v) + 1
    return torch.Generator().manual_seed(s % (2 ** 31))


@dataclasses.dataclass(frozen=True)
class Case:
    M: int
    N: int
    K: int
    a_col: bool = False
    b_col: bool = False
    S: int = 1
    outs: tuple = ("c32",)          # of "c" (bf16 out), "c32" (fp32 slabs), "c2" (bf16 out2)
    ldc32: int = -1                 # -1: N + 8, or N rounded up to 4 when N % 8
    csum: bool = False              # column sums of A in column N of every slab
    bias: str = ""                  # "vec": contiguous [N]; "col": a column of a matrix
    relu: bool = False
    mask: bool = False
    mul: bool = False
    add: bool = False
    pitch: str = "pad"              # container of out / mask, see _out_slot
    seed: int = 0
    a_from: "Case | None" = None    # stored A shared with this case (a layer's dy)

    @property
    def ld32(self):
        if self.ldc32 >= 0:
            return self.ldc32
        return _up(self.N, 4) if self.N % 8 else self.N + 8

    @property
    def ktiles(self):
        return (self.K + 63) // 64

    def empty_slabs(self):
        per = -(-self.ktiles // self.S)
        return [z for z in range(self.S) if z * per >= self.ktiles]


def case_id(c):
    s = f"{'c' if c.a_col else 'r'}{'c' if c.b_col else 'r'}-{c.M}x{c.N}x{c.K}"
    if c.S > 1 or c.ldc32 >= 0:
        s += f"-s{c.S}"
    s += "-" + "+".join(c.outs)
    for flag, name in ((c.csum, "csum"), (c.bias, "bias" + c.bias), (c.relu, "relu"),
                       (c.mask, "mask"), (c.mul, "mul"), (c.add, "add")):
        if flag:
            s += "-" + name
    if c.pitch != "pad":
        s += "-" + c.pitch
    return s


# ------------------------------------------------------------- containers
class Slot:
    """A strided view (off, size, stride) into a flat parent of ``numel``."""

    def __init__(self, numel, off, size, stride, dtype):
        self.numel, self.off, self.size, self.stride, self.dtype = numel, off, size, stride, dtype
        last = off + sum((n - 1) * s for n, s in zip(size, stride))
        assert 0 < off and last < numel

    def parent(self, fill, device="cpu"):
        return torch.full((self.numel,), fill, dtype=self.dtype, device=device)

    def view(self, parent):
        return parent.as_strided(self.size, self.stride, self.off)


def _operand_slot(R, C):
    """bf16 [R, C] operand: 2 rows before, 1 after, 8 columns before and >= 8
    after; 16-B aligned origin, pitch a multiple of 8."""
    pitch = _up(C, 8) + 16
    return Slot((R + 3) * pitch + 16, 2 * pitch + 8, (R, C), (pitch, 1), torch.bfloat16)


def _out_slot(M, N, pitch):
    """bf16 [M, N] out / out2 / mask / mul / add container, >= 1 row + 8
    columns before and after.
      pad:    pitch N rounded up to 8, + 8; rows 16-B aligned
      n8:     pitch N + 8, 16-B aligned base
      odd:    pitch N + 3, base one column off: 2-B aligned
      contig: pitch N (what linear_fwd allocates), 16-B aligned base"""
    ld = {"pad": _up(N, 8) + 8, "n8": N + 8, "odd": N + 3, "contig": N}[pitch]
    off = _up(ld, 8) + 8 + (1 if pitch == "odd" else 0)
    return Slot(off + M * ld + ld + 8, off, (M, N), (ld, 1), torch.bfloat16)


def _c32_slot(c):
    lead = _up(c.ld32 + 8, 4)
    n = c.S * c.M * c.ld32
    return Slot(lead + n + lead, lead, (n,), (1,), torch.float32)


def _bias_slot(N, kind):
    if kind == "vec":
        return Slot(N + 12, 4, (N,), (1,), torch.float32)
    P = 12                                         # a column of an [N + 2, 12] matrix
    return Slot((N + 2) * P, P + 3, (N,), (P,), torch.float32)


# ------------------------------------------------------------------ inputs
@functools.lru_cache(maxsize=None)
def case_data(c, mode):
    """Logical float64 operands + their containers (slot, cached CPU parent)."""
    assert mode in ("exact", "float")
    g = _gen(mode == "float", c.M, c.N, c.K, c.a_col, c.b_col, c.S, c.seed)

    def draw(*shape):
        if mode == "exact":
            return torch.randint(-3, 4, shape, generator=g).double()
        return torch.randn(shape, generator=g).bfloat16().double()

    def put(slot, logical):
        p = slot.parent(float("nan"))
        slot.view(p).copy_(logical)
        assert torch.equal(slot.view(p).double().nan_to_num(nan=123.0),
                           logical.nan_to_num(nan=123.0)), "not representable"
        return slot, p

    d, ins = {}, {}
    if c.a_from is not None:
        o = case_data(c.a_from, mode)
        d["A_store"], ins["a"] = o["A_store"], o["in"]["a"]
    else:
        d["A_store"] = draw(c.K, c.M) if c.a_col else draw(c.M, c.K)
        ins["a"] = put(_operand_slot(*d["A_store"].shape), d["A_store"])
    d["A"] = d["A_store"].t() if c.a_col else d["A_store"]              # [M, K]
    assert d["A"].shape == (c.M, c.K)
    d["B_store"] = draw(c.K, c.N) if c.b_col else draw(c.N, c.K)
    ins["b"] = put(_operand_slot(*d["B_store"].shape), d["B_store"])
    d["B"] = d["B_store"] if c.b_col else d["B_store"].t()              # [K, N]
    if c.bias:
        d["bias"] = (torch.randint(-16, 17, (c.N,), generator=g).double() / 4 if mode == "exact"
                     else torch.randn(c.N, generator=g).double())
        ins["bias"] = put(_bias_slot(c.N, c.bias), d["bias"])
    if c.mask:
        tab = torch.tensor(MASK_TABLE, dtype=torch.float64)
        d["mask"] = tab[torch.randint(0, len(MASK_TABLE), (c.M, c.N), generator=g)]
        ins["mask"] = put(_out_slot(c.M, c.N, c.pitch), d["mask"])
        if c.M * c.N >= 1000:
            assert float((d["mask"] == 0).double().mean()) >= 1 / 3
            assert bool((d["mask"] == BF16_MIN_SUBNORMAL).any())
    for name, on in (("mul", c.mul), ("add", c.add)):
        if on:
            d[name] = draw(c.M, c.N)
            ins[name] = put(_out_slot(c.M, c.N, "pad"), d[name])
    outs = {}
    if "c" in c.outs:
        outs["c"] = _out_slot(c.M, c.N, c.pitch)
    if "c2" in c.outs:
        outs["c2"] = _out_slot(c.M, c.N, "pad")
    if "c32" in c.outs:
        outs["c32"] = _c32_slot(c)
    assert not (c.csum and not (c.a_col and "c32" in c.outs and c.ld32 > c.N))
    d["in"], d["out"] = ins, outs
    return d


# ------------------------------------------------------------------ oracle
@functools.lru_cache(maxsize=None)
def gemm_oracle(c, mode):
    """Exact float64 values and magnitudes of everything ``c`` asks for."""
    d = case_data(c, mode)
    A, B = d["A"], d["B"]
    x = A @ B
    T = A.abs() @ B.abs()
    if c.bias:
        x = x + d["bias"]
        T = T + d["bias"].abs()
    v = x.clamp_min(0) if c.relu else x
    live = torch.ones(c.M, c.N, dtype=torch.bool)
    if c.mask:
        live = d["mask"] > 0                      # False for NaN, -0.0, +0.0
        v = torch.where(live, v, torch.zeros_like(v))
    mul = d["mul"] if c.mul else torch.ones_like(v)
    add = d["add"] if c.add else torch.zeros_like(v)
    o = {"case": c, "mode": mode, "v": v, "T": T, "live": live, "c2": v * mul + add,
         "mul": mul, "add": add, "csum": A.sum(1), "csum_mag": A.abs().sum(1)}
    if mode == "exact":
        # the exactness argument of the module docstring, for this very case
        assert c.K <= EXACT_MAX_K
        big = max(float(T.max()), float(o["c2"].abs().max()), float((T * mul.abs()).max()))
        assert big < EXACT_LIMIT, big
        assert bool(((v * 4) == (v * 4).round()).all())
    return o


def rne_bf16(x):
    """float64 -> nearest bf16 (ties to even), as float64."""
    return x.float().bfloat16().double()


def bounds(o):
    """Float-mode bounds of the module docstring -> {c32, c, c2, csum}."""
    c = o["case"]
    n = (c.K + c.S + 2) * U23
    acc = torch.where(o["live"], n * o["T"], torch.zeros_like(o["T"]))
    e2 = o["mul"].abs() * acc + 2 * U23 * ((o["v"] * o["mul"]).abs() + o["add"].abs())
    return {"c32": acc, "c": acc + U8 * (o["v"].abs() + acc),
            "c2": e2 + U8 * (o["c2"].abs() + e2), "csum": n * o["csum_mag"]}


def compare(got, exact, bound, mode, bf16, what):
    """Exact mode: got == exact (fp32) or == its bf16 rounding, no tolerance.
    Float mode: |got - exact| <= bound everywhere. An element that is still
    NaN (never written) fails both. Returns the worst error / bound ratio."""
    got = got.detach().cpu().double()
    assert got.shape == exact.shape, (what, got.shape, exact.shape)
    if mode == "exact":
        want = rne_bf16(exact) if bf16 else exact
        bad = ~(got == want)
        assert not bool(bad.any()), (what, int(bad.sum()), bad.nonzero()[0].tolist(),
                                     float(got[bad][0]), float(want[bad][0]))
        return 0.0
    err = (got - exact).abs()
    bad = ~(err <= bound)
    assert not bool(bad.any()), (what, int(bad.sum()), bad.nonzero()[0].tolist(),
                                 float(err[bad][0]), float(bound[bad][0]))
    nz = bound > 0
    return float((err[nz] / bound[nz]).max()) if bool(nz.any()) else 0.0


def check_gemm(got, o, mode, slab0=False):
    """``got``: {"c" | "c2" | "c32": the output's whole parent after the call}.
    Every requested element within its bound (exact mode: equal), none left
    unwritten, every parent element outside the written region still the
    sentinel, empty slabs all zeros. ``slab0``: the CPU reference's documented
    split semantics (slab 0 holds everything, the others zeros). Returns the
    worst error / bound ratio (0 in exact mode)."""
    c = o["case"]
    assert mode == o["mode"] and set(got) == set(c.outs)
    slots = case_data(c, mode)["out"]
    bd = bounds(o)
    worst = 0.0
    for name in ("c", "c2"):
        if name not in got:
            continue
        p = got[name].detach().cpu()
        worst = max(worst, compare(slots[name].view(p), o["v" if name == "c" else name],
                                   bd[name], mode, True, name))
        ring = p.clone()
        slots[name].view(ring).fill_(SENTINEL)
        assert bool((ring == SENTINEL).all()), f"{name}: written outside [M, N]"
    if "c32" in got:
        p = got["c32"].detach().cpu()
        sl = slots["c32"].view(p).view(c.S, c.M, c.ld32)
        body = sl[:, :, :c.N].double()
        assert not bool(body.isnan().any()), "c32: a slab element was never written"
        worst = max(worst, compare(body.sum(0), o["v"], bd["c32"], mode, False, "c32"))
        zero = list(range(1, c.S)) if slab0 else c.empty_slabs()
        for z in zero:
            assert bool((sl[z, :, :c.N] == 0).all()), f"c32: empty slab {z} is not zero"
        if c.csum:
            col = sl[:, :, c.N].double()
            assert not bool(col.isnan().any()), "csum: a slab's column was never written"
            worst = max(worst, compare(col.sum(0), o["csum"], bd["csum"], mode, False, "csum"))
            for z in zero:
                assert bool((col[z] == 0).all()), f"csum: empty slab {z} is not zero"
        ring = p.clone()
        rs = slots["c32"].view(ring).view(c.S, c.M, c.ld32)
        rs[:, :, :c.N] = SENTINEL
        if c.csum:
            rs[:, :, c.N] = SENTINEL
        assert bool((ring == SENTINEL).all()), "c32: written outside the slabs' [M, N] (+ csum)"
    return worst


# ----------------------------------------------------------------- running
def fresh_outputs(c, mode, device="cpu"):
    """Output parents: SENTINEL everywhere, NaN where the op must write."""
    out = {}
    for name, slot in case_data(c, mode)["out"].items():
        p = slot.parent(SENTINEL, device)
        if name == "c32":
            sl = slot.view(p).view(c.S, c.M, c.ld32)
            sl[:, :, :c.N] = float("nan")
            if c.csum:
                sl[:, :, c.N] = float("nan")
        else:
            slot.view(p).fill_(float("nan"))
        out[name] = p
    return out


def compose(c, mode, values):
    """Output parents as a run that computed ``values`` would leave them:
    {c, c2: [M, N]; c32: [S, M, N]; csum: [S, M]} float64 (bf16 outputs are
    rounded to nearest even on the way in)."""
    outp = fresh_outputs(c, mode)
    slots = case_data(c, mode)["out"]
    for name, p in outp.items():
        if name == "c32":
            sl = slots[name].view(p).view(c.S, c.M, c.ld32)
            sl[:, :, :c.N] = values["c32"].float()
            if c.csum:
                sl[:, :, c.N] = values["csum"].float()
        else:
            slots[name].view(p).copy_(values[name].float())
    return outp


def stage(c, mode, device):
    """-> (input views on ``device``, output parents on ``device``)."""
    d = case_data(c, mode)
    ins = {k: slot.view(p.to(device)) for k, (slot, p) in d["in"].items()}
    return ins, fresh_outputs(c, mode, device)


def launch(c, mode, ins, outp):
    slots = case_data(c, mode)["out"]
    view = {k: slots[k].view(p) for k, p in outp.items()}
    ops.gemm(ins["a"], c.a_col, ins["b"], c.b_col, ins.get("bias"), c.relu, ins.get("mask"),
             view.get("c"), view.get("c32"), c.S, ins.get("mul"), ins.get("add"), view.get("c2"),
             c.ld32 if "c32" in view else 0, c.N if c.csum else -1)


def _finish(outp):
    return {k: p.cpu() for k, p in outp.items()}


def run_gemm(c, device, policy=None, mode="exact"):
    """One ``ops.gemm`` of case ``c`` on ``device`` (policy: GEMM tile policy
    for the call, restored after) -> the output parents, on the CPU."""
    ins, outp = stage(c, mode, device)
    old = ops.gemm_policy(policy) if policy is not None else None
    try:
        launch(c, mode, ins, outp)
    finally:
        if policy is not None:
            ops.gemm_policy(old)
    return _finish(outp)


def run_pair(cases, device, policy=None, mode="exact", pairing=1):
    """The cases' GEMMs recorded under one ``ops.gemm_batch`` (GPU; on the CPU
    they simply run in order) -> [output parents per case]."""
    gpu = torch.device(device).type == "cuda"
    staged = [stage(c, mode, device) for c in cases]
    oldp = ops.gemm_policy(policy) if policy is not None else None
    oldq = ops.gemm_pairing(pairing) if gpu else None
    try:
        with ops.gemm_batch(enabled=gpu):
            for c, (ins, outp) in zip(cases, staged):
                launch(c, mode, ins, outp)
    finally:
        if gpu:
            ops.gemm_pairing(oldq)
        if policy is not None:
            ops.gemm_policy(oldp)
    return [_finish(outp) for _, outp in staged]


def plain_inputs(c, mode, device):
    """Contiguous device copies of the stored operands, for the wrappers that
    allocate their own outputs: {a, b, bias, mask}."""
    d = case_data(c, mode)
    out = {"a": d["A_store"].to(torch.bfloat16).to(device),
           "b": d["B_store"].to(torch.bfloat16).to(device)}
    if c.bias:
        out["bias"] = d["bias"].float().to(device)
    if c.mask:
        out["mask"] = d["mask"].to(torch.bfloat16).to(device)
    return out


# ------------------------------------------------------------------- cases
RR, RC, CC = (False, False), (False, True), (True, True)
LAYOUTS = (RR, RC, CC)


def _allowed(M, N, lay):
    return not (lay[0] and M % 8) and not (lay[1] and N % 8)


def _mk(M, N, K, lay, **kw):
    assert _allowed(M, N, lay)
    return Case(M, N, K, lay[0], lay[1], **kw)


# (M, N) at K = 192: one block, tails in M and N, several blocks, a 256-row
# tile whose second 128-row image is almost all clamped (264) or partial (392)
SHAPES_ALL = ((8, 8), (64, 128), (72, 136), (120, 120), (128, 128), (136, 264), (256, 128),
              (264, 136), (392, 8))
SHAPES_ROW_A = ((1, 8), (37, 72))
SHAPES_RR = ((1, 1), (37, 1), (130, 7), (65, 20), (129, 133), (257, 129))
# policy 1 gives a row-layout A the 128-row two-stage body only from 256
# 128x128 tiles up (below that the 64-row one): 2 x 128 tiles, one K tile
SHAPES_WIDE = ((136, 16384),)
SHAPE_CASES = tuple(
    [_mk(M, N, 192, lay, outs=("c", "c32")) for M, N in SHAPES_ALL for lay in LAYOUTS]
    + [_mk(M, N, 192, lay, outs=("c", "c32")) for M, N in SHAPES_ROW_A for lay in (RR, RC)]
    + [_mk(M, N, 192, RR, outs=("c", "c32")) for M, N in SHAPES_RR]
    + [_mk(M, N, 64, lay, outs=("c", "c32")) for M, N in SHAPES_WIDE for lay in (RR, RC)])

# 1..7 K tiles (prologue only, steady state, drain, one full wrap of the 2-,
# 3- and 4-deep rings) and the K tails the binding zero-pads. For a K tail the
# binding copies A and B into zero-padded tensors of their own, so there the
# NaN parents guard nothing: those cases check the padding, not stray reads.
K_SWEEP = (64, 128, 192, 256, 320, 448, 16, 100, 200)
K_CASES = tuple(_mk(136, 136, K, lay) for K in K_SWEEP for lay in LAYOUTS)

# split-K: fp32 slabs of pitch N + 64, with and without the A column sums;
# 5 K tiles in 4 splits leaves the last slab empty (2, 2, 1, 0)
SPLITS = ((136, 136, 320, 1), (136, 136, 320, 2), (136, 136, 320, 4), (136, 136, 320, 5),
          (264, 128, 128, 2), (8, 264, 448, 3))
SPLIT_CASES = tuple(
    [_mk(M, N, K, CC, S=S, ldc32=N + 64, csum=cs) for M, N, K, S in SPLITS for cs in (False, True)]
    + [_mk(136, 136, 320, RC, S=2, ldc32=136 + 64)])
assert Case(136, 136, 320, True, True, S=4).empty_slabs() == [3]

_EPI = (dict(outs=("c32",)),
        dict(outs=("c",)),
        dict(outs=("c", "c32"), bias="vec", relu=True),
        dict(outs=("c",), bias="col"),
        dict(outs=("c",), mask=True),
        dict(outs=("c",), bias="vec", relu=True, mask=True),
        dict(outs=("c", "c2"), mul=True, add=True),
        dict(outs=("c2",), mul=True),
        dict(outs=("c2",), add=True, mask=True, relu=True),
        dict(outs=("c2",)))
# (256, 128): one full tile, the register-direct paths
EPI_SHAPES = ((136, 264), (129, 133), (256, 128))
EPI_CASES = tuple(
    [_mk(M, N, 128, RR, seed=1, **kw) for M, N in EPI_SHAPES for kw in _EPI]
    # the dgrad layout for the mask and second-output variants
    + [_mk(M, N, 128, RC, seed=1, **kw) for M, N in EPI_SHAPES if N % 8 == 0 for kw in _EPI[4:]])

# out and mask at pitches / bases that are not 16-B aligned (all accepted by
# the binding). With a mask the shared epilogue() of the two-stage, deep and
# 256x128 kernels stages the tile through LDS and moves every whole 8-column
# group as one 16-B access at whatever address that is: N = 264 prefetches the
# mask that way and stores 33 groups per row; N = 20 loads and stores groups
# 0-7 and 8-15 that way and takes the scalar tail for columns 16-19.
# pp_epilogue (ping-pong and two-group kernels) goes element by element for
# the odd pitch and for N = 20 (pitch % 8 != 0), as it does for every partial
# wave tile; at N = 264 the n8 and contig containers are 16-B aligned with
# pitch % 8 == 0, so full wave tiles keep its vector path.
PITCH_CASES = tuple(_mk(M, N, 128, RR, seed=2, outs=("c",), bias="vec", relu=True, mask=True,
                        pitch=p)
                    for M, N in ((136, 264), (65, 20)) for p in ("n8", "odd", "contig"))

# the cases the teeth tests corrupt: every epilogue stage and all three
# outputs at once; a two-slab weight grad with column sums
TEETH_EPI = _mk(136, 264, 128, RR, seed=9, outs=("c", "c32", "c2"), bias="vec", relu=True,
                mask=True, mul=True, add=True)
TEETH_SPLIT = _mk(136, 136, 320, CC, S=2, ldc32=136 + 64, csum=True)
assert TEETH_SPLIT in SPLIT_CASES

# the GPU float-mode subset: the K sweep, the splits, three epilogues
FLOAT_CASES = K_CASES + SPLIT_CASES + (EPI_CASES[5], EPI_CASES[6], EPI_CASES[18])
assert EPI_CASES[5].mask and EPI_CASES[6].mul and EPI_CASES[18].N == 133 and EPI_CASES[18].add

# Pairs under ops.gemm_batch. A pair forms only when both problems land on
# the same kernel family (gemm.hip try_pair): ping-pong + ping-pong, 256x128 +
# 256x128 (or + a deep-kernel dgrad, moved over), two-group + two-group; a
# weight grad with column sums always runs on the ping-pong kernel. So:
#   csum:  out width 264, in width 136, batch 320: dW = dy^T x with the
#          column sums of dy, dx = dy W masked by x's ReLU. Pairs on the
#          ping-pong pair kernel under policies 0 and 3 (grids 3 x 2 x 2
#          against 3 x 2). The dgrad's K = 264 is a tail, so the binding hands
#          the kernel a padded copy of dy, not the weight grad's buffer.
#   layer: the same without column sums, out width 384, batch 320 (both
#          multiples of 64: one dy buffer read by both). Ping-pong pair under
#          0 and 3, 256x128 pair under 4 and 5 (2 x 2 x 2 against 2 x 2
#          256-row tiles, each with a partial second half), two-group pair
#          under 8.
#   two:   two weight grads, M = 264 (a 256-row tile + 8 rows) with 2 splits
#          and 5 K tiles in 4 splits (an empty slab inside a pair grid); the
#          same kernels as "layer".
#   long:  float mode only (K = 1024 is past the exact-mode limit): under
#          policy 5 the dgrad alone would take the deep kernel (16 K tiles)
#          and moves onto the 256x128 pair kernel beside its weight grad;
#          ping-pong pair under 0 and 3.
# Policies 1 and 2 never pair. Every member also runs unpaired under every
# policy (ALL_CASES).
PAIR_WGRAD = Case(264, 136, 320, True, True, S=2, ldc32=136 + 64, csum=True, seed=3)
PAIR_DGRAD = Case(320, 136, 264, False, True, outs=("c",), mask=True, seed=3, a_from=PAIR_WGRAD)
LAYER_WGRAD = Case(384, 136, 320, True, True, S=2, ldc32=136 + 64, seed=6)
LAYER_DGRAD = Case(320, 136, 384, False, True, outs=("c",), mask=True, seed=6, a_from=LAYER_WGRAD)
TWO_WGRAD_A = Case(264, 136, 320, True, True, S=2, ldc32=136 + 64, seed=4)
TWO_WGRAD_B = Case(136, 264, 320, True, True, S=4, ldc32=264 + 64, seed=4)
LONG_WGRAD = Case(1024, 136, 128, True, True, S=2, ldc32=136 + 64, seed=7)
LONG_DGRAD = Case(128, 136, 1024, False, True, outs=("c",), mask=True, seed=7, a_from=LONG_WGRAD)
PAIRS = {"csum": (PAIR_WGRAD, PAIR_DGRAD), "layer": (LAYER_WGRAD, LAYER_DGRAD),
         "two": (TWO_WGRAD_A, TWO_WGRAD_B), "long": (LONG_WGRAD, LONG_DGRAD)}
PAIR_MODES = {"csum": ("exact", "float"), "layer": ("exact", "float"), "two": ("exact", "float"),
              "long": ("float",)}
# (pair, policy) for which a paired launch forms
PAIR_RUNS = tuple([("csum", p) for p in (0, 3)]
                  + [(n, p) for n in ("layer", "two") for p in (0, 3, 4, 5, 8)]
                  + [("long", p) for p in (0, 3, 5)])

ALL_CASES = (SHAPE_CASES + K_CASES + SPLIT_CASES + EPI_CASES + PITCH_CASES + (TEETH_EPI,)
             + PAIRS["csum"] + PAIRS["layer"] + PAIRS["two"])
assert len(set(ALL_CASES)) == len(ALL_CASES)

# the wrappers: linear_fwd into a 20-wide layer, its dgrad, a weight grad
WRAP_FWD = Case(65, 20, 128, False, False, outs=("c",), bias="vec", relu=True, seed=5)
WRAP_DGRAD = Case(65, 136, 72, False, True, outs=("c",), mask=True, seed=5)
WRAP_WGRAD = Case(72, 136, 320, True, True, seed=5)
WGRAD_MODES = ((None, False), (3, False), (3, True), (1, True))     # (splits, accumulate)


def wgrad_init(c, mode):
    """The non-zero ``out`` an accumulating weight grad adds to, float64."""
    g = _gen(77, mode == "float", c.M, c.N)
    if mode == "exact":
        return torch.randint(-3, 4, (c.M, c.N), generator=g).double()
    return torch.randn(c.M, c.N, generator=g).float().double()


def wgrad_bound(o, S, init, accumulate):
    """linear_wgrad (module docstring): acc for S splits, whose S - 1 slab
    additions it already counts; accumulating adds one term, ``init``."""
    c = o["case"]
    if not accumulate:
        return (c.K + S + 2) * U23 * o["T"]
    return (c.K + S + 3) * U23 * (o["T"] + init.abs())


def check_wrappers(device, mode):
    """linear_fwd / linear_dgrad / linear_wgrad (shared with the GPU tests)."""
    worst = 0.0
    c = WRAP_FWD
    o, t = gemm_oracle(c, mode), plain_inputs(c, mode, device)
    y = ops.linear_fwd(t["a"], t["b"], t["bias"], relu=True)
    assert y.shape == (c.M, c.N) and y.is_contiguous()
    worst = max(worst, compare(y, o["v"], bounds(o)["c"], mode, True, "linear_fwd"))
    c = WRAP_DGRAD
    o, t = gemm_oracle(c, mode), plain_inputs(c, mode, device)
    dx = ops.linear_dgrad(t["a"], t["b"], mask=t["mask"])
    worst = max(worst, compare(dx, o["v"], bounds(o)["c"], mode, True, "linear_dgrad"))
    c = WRAP_WGRAD
    o, t = gemm_oracle(c, mode), plain_inputs(c, mode, device)
    init = wgrad_init(c, mode)
    for splits, accumulate in WGRAD_MODES:
        out = init.float().to(device).reshape(-1).clone()
        ops.linear_wgrad(t["a"], t["b"], out, splits=splits, accumulate=accumulate)
        exact = o["v"] + init if accumulate else o["v"]
        worst = max(worst, compare(out.view(c.M, c.N), exact,
                                      wgrad_bound(o, splits or 1, init, accumulate), mode,
                                      False,
                                      f"linear_wgrad splits={splits} accumulate={accumulate}"))
    return worst


def worst_ratio_line(tag, worst):
    return f"dense-oracle worst error/bound [{tag}]: {worst:.4f}"
